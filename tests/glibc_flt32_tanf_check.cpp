// tests/glibc_flt32_tanf_check.cpp -- CPU check of icar_amd/csrc/glibc_flt32_tan.h (the device's tanf) against the host C
// library, value by value.  Built and run by tests/test_glibc_flt32_tanf_host.py:
//     g++ -O2 -ffp-contract=off -fopenmp glibc_flt32_tanf_check.cpp -o ... ;  ./check <stride>
// Every REAL(4) bit pattern whose index is a multiple of <stride> (1 = all 2^32).  Prints "tanf <tested> <mismatches>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define GF_FN static inline
#define GF_TABLE static const
#include "../icar_amd/csrc/glibc_flt32_tan.h"

static inline bool same(float a, float b)
{
    if (std::isnan(a) && std::isnan(b)) return true;
    return gf_asuint(a) == gf_asuint(b);
}

int main(int argc, char **argv)
{
    const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
    if (stride == 0) return 2;
    uint64_t bad = 0, n = 0; uint32_t first = 0; bool have = false;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
    for (int64_t b = 0; b < (int64_t)1 << 32; b += (int64_t)stride) {
        const float x = gf_asfloat((uint32_t)b);
        ++n;
        if (!same(gf_tanf(x), tanf(x))) {
            ++bad;
#pragma omp critical
            if (!have || (uint32_t)b < first) { have = true; first = (uint32_t)b; }
        }
    }
    printf("tanf %llu %llu", (unsigned long long)n, (unsigned long long)bad);
    if (have) { const float x = gf_asfloat(first); printf("  first: x=%a mine=%a ref=%a", x, gf_tanf(x), tanf(x)); }
    printf("\n");
    return 0;
}

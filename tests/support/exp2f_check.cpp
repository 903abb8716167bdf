// tests/support/exp2f_check.cpp -- CPU check of gf_exp2f (icar_amd/csrc/glibc_flt32.h: the device's exp2f, which the Noah cell code
// needs for 2.0 ** x) against the host C library, value by value.  Built and run by tests/test_exp2f_host.py:
//     g++ -O2 -mfma -ffp-contract=off -fopenmp exp2f_check.cpp -o ... ;  ./check <stride>
// Every REAL(4) bit pattern whose index is a multiple of <stride> (1 = all 2^32).  Prints "exp2f <tested> <mismatches>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define GF_FN static inline
#define GF_TABLE static const
#include "../../icar_amd/csrc/glibc_flt32.h"

int main(int argc, char **argv)
{
    const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
    uint64_t bad = 0, n = 0; uint32_t first = 0; bool have = false;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
    for (int64_t b = 0; b < (int64_t)1 << 32; b += (int64_t)stride) {
        const float x = gf_asfloat((uint32_t)b);
        const float mine = gf_exp2f(x), ref = exp2f(x);
        ++n;
        if (!((std::isnan(mine) && std::isnan(ref)) || gf_asuint(mine) == gf_asuint(ref))) {
            ++bad;
#pragma omp critical
            if (!have) { have = true; first = (uint32_t)b; }
        }
    }
    printf("exp2f %llu %llu", (unsigned long long)n, (unsigned long long)bad);
    if (have) { const float x = gf_asfloat(first); printf("  first: x=%a mine=%a ref=%a", x, gf_exp2f(x), exp2f(x)); }
    printf("\n");
    return 0;
}

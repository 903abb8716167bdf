// tests/glibc_flt32_trig_check.cpp -- CPU check of icar_amd/csrc/glibc_flt32_trig.h (the device's sinf / cosf / asinf) against
// the host C library, value by value.  Built and run by tests/test_glibc_flt32_trig_host.py:
//     g++ -O2 -mfma -ffp-contract=off -fopenmp glibc_flt32_trig_check.cpp -o ... ;  ./check <stride>
// Every REAL(4) bit pattern whose index is a multiple of <stride> (1 = all 2^32).  "sincosf" compares the C library's sincosf
// with its own sinf / cosf on the same arguments (the compiled reference calls all three).  Prints
// "<name> <tested> <mismatches>" per function.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define GF_FN static inline
#define GF_TABLE static const
#include "../icar_amd/csrc/glibc_flt32_trig.h"

static inline bool same(float a, float b)
{
    if (std::isnan(a) && std::isnan(b)) return true;
    return gf_asuint(a) == gf_asuint(b);
}

template <class F, class G>
static void sweep(const char *name, F mine, G ref, uint64_t stride)
{
    uint64_t bad = 0, n = 0; uint32_t first = 0; bool have = false;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
    for (int64_t b = 0; b < (int64_t)1 << 32; b += (int64_t)stride) {
        const float x = gf_asfloat((uint32_t)b);
        ++n;
        if (!same(mine(x), ref(x))) {
            ++bad;
#pragma omp critical
            if (!have) { have = true; first = (uint32_t)b; }
        }
    }
    printf("%s %llu %llu", name, (unsigned long long)n, (unsigned long long)bad);
    if (have) { const float x = gf_asfloat(first); printf("  first: x=%a mine=%a ref=%a", x, mine(x), ref(x)); }
    printf("\n");
}

// sincosf's two results packed into one comparison: the sine when both agree with sinf / cosf, otherwise a NaN / number mix
static float sincos_sin(float x) { float s, c; sincosf(x, &s, &c); return s; }
static float sincos_cos(float x) { float s, c; sincosf(x, &s, &c); return c; }

int main(int argc, char **argv)
{
    const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
    sweep("sinf", gf_sinf, [](float x) { return sinf(x); }, stride);
    sweep("cosf", gf_cosf, [](float x) { return cosf(x); }, stride);
    sweep("asinf", gf_asinf, [](float x) { return asinf(x); }, stride);
    sweep("sincosf_sin", sincos_sin, [](float x) { return sinf(x); }, stride);
    sweep("sincosf_cos", sincos_cos, [](float x) { return cosf(x); }, stride);
    return 0;
}

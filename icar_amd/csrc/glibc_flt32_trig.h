// icar_amd/csrc/glibc_flt32_trig.h -- sinf / cosf / asinf exactly as the compiled reference evaluates them (sibling of
// glibc_flt32.h, same GF_FN / GF_TABLE conventions).
// Origin and licence: restated from the GNU C Library 2.35 (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, s_sincosf.h,
// s_sincosf_data.c: Copyright (C) Free Software Foundation, Inc. / Arm Ltd., "optimized routines"; e_asinf.c: Copyright (C) 1993
// Sun Microsystems, Inc. (fdlibm), with glibc's degree-4 polynomial), GNU Lesser General Public License 2.1 or later (the Arm
// originals also MIT; fdlibm: "permission to use, copy, modify, and distribute this software is freely granted, provided that
// this notice is preserved").  The algorithms and constants are theirs; this file is a derived work under the same terms.
//
// flang lowers REAL(4) sin / cos / asin to sinf / cosf / asinf (and a sin + cos pair of one argument to sincosf, which gives
// the same two values: s_sincosf.c evaluates the same two polynomials on the same reduced argument; checked on every argument
// by tests/glibc_flt32_trig_check.cpp).  sinf / cosf: one reduction to [-pi/4, pi/4] in double precision (|x| < 120: a
// multiply by 2/pi; above: 192 bits of 4/pi, so the contract is the whole REAL(4) line) and a degree-7 / degree-8 polynomial in
// double, rounded once.  x86-64 glibc selects its FMA builds of the three at load time (AVX2 + FMA); they contract every
// a * b + c of the source, written below as fma().  asinf has no FMA build: plain float arithmetic and one IEEE square root.
// Checked value by value on all 2^32 arguments against the host's libm (tests/test_glibc_flt32_trig_host.py) and on the
// device (tests/test_gpu_trig_math.py).
#pragma once
#include "glibc_flt32.h"

// __sincosf_table[0]'s polynomials (table [1] is the same with c0..c4 negated: here the sign is applied to the result, which
// gives the same bits because negation commutes with every rounding) and __inv_pio4: 4/pi to 192 bits, 8 new bits per entry
struct GfTrigTab { uint32_t inv_pio4[24]; };
GF_TABLE GfTrigTab gf_trig_tab = {{
    0xa2, 0xa2f9, 0xa2f983, 0xa2f9836e, 0xf9836e4e, 0x836e4e44, 0x6e4e4415, 0x4e441529, 0x441529fc, 0x1529fc27, 0x29fc2757, 0xfc2757d1,
    0x2757d1f5, 0x57d1f534, 0xd1f534dd, 0xf534ddc0, 0x34ddc0db, 0xddc0db62, 0xc0db6295, 0xdb629599, 0x6295993c, 0x95993c43, 0x993c4390, 0x3c439041}};

GF_FN uint32_t gf_abstop12(float x) { return (gf_asuint(x) >> 20) & 0x7ff; }

// sinf_poly (s_sincosf.h): sin(x) for even n, cos(x) for odd n, x in [-pi/4, pi/4], x2 = x * x
GF_FN double gf_sin_poly(double x, double x2)
{
    const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    const double x3 = x * x2;
    const double s1 = __builtin_fma(x2, S3, S2);
    const double x7 = x3 * x2;
    const double s = __builtin_fma(x3, S1, x);
    return __builtin_fma(x7, s1, s);
}
GF_FN double gf_cos_poly(double x2)
{
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10, C4 = 0x1.99343027bf8c3p-16;
    const double x4 = x2 * x2;
    const double c2 = __builtin_fma(x2, C4, C3);
    const double c1 = __builtin_fma(x2, C1, C0);
    const double x6 = x4 * x2;
    const double c = __builtin_fma(x4, C2, c1);
    return __builtin_fma(x6, c2, c);
}

// reduce_fast: |x| < 120.  n = round(x * 2/pi) through a scaled truncation; returns x - n * pi/2
GF_FN double gf_reduce_fast(double x, int *np)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const double r = x * hpi_inv;
    const int n = ((int32_t)r + 0x800000) >> 24;
    *np = n;
    return __builtin_fma(-(double)n, hpi, x);
}
// reduce_large: 120 <= |x| < inf from the bit pattern: |x| * 4/pi mod 8 in 64-bit fixed point
GF_FN double gf_reduce_large(uint32_t xi, int *np)
{
    const uint32_t *arr = &gf_trig_tab.inv_pio4[(xi >> 26) & 15];
    const int shift = (xi >> 23) & 7;
    xi = (xi & 0xffffff) | 0x800000;
    xi <<= shift;
    uint64_t res0 = (uint32_t)(xi * arr[0]);
    const uint64_t res1 = (uint64_t)xi * arr[4];
    const uint64_t res2 = (uint64_t)xi * arr[8];
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    const uint64_t n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    const double x = (double)(int64_t)res0;
    *np = (int)n;
    return x * 0x1.921FB54442D18p-62;
}

// both functions: reduce, then quadrant q = n (+ sign of x above 120) selects the polynomial and the sign
//   sign[q & 3] = {1, -1, -1, 1} multiplies the reduced x; (q & 2) negates the cosine polynomial
GF_FN float gf_sincos_reduced(float y, int want_cos)
{
    double x = (double)y;
    int n, q;
    if (gf_abstop12(y) < 0x42f) { x = gf_reduce_fast(x, &n); q = n; }           // abstop12(120.0f)
    else { const uint32_t xi = gf_asuint(y); x = gf_reduce_large(xi, &n); q = n + (int)(xi >> 31); }
    const double s = ((q + 1) & 2) ? -1.0 : 1.0;
    if ((n ^ want_cos) & 1) { const double c = gf_cos_poly(x * x); return (float)((q & 2) ? -c : c); }
    return (float)gf_sin_poly(x * s, x * x);
}

GF_FN float gf_sinf(float y)
{
    const uint32_t t = gf_abstop12(y);
    if (t < 0x3f4) {                                            // |y| < pi/4  (abstop12(0x1.921FB6p-1f))
        if (GF_UNLIKELY(t < 0x398)) return y;                   // |y| < 2^-12
        const double x = (double)y;
        return (float)gf_sin_poly(x, x * x);
    }
    if (GF_UNLIKELY(t >= 0x7f8)) return (y - y) / (y - y);      // inf, NaN
    return gf_sincos_reduced(y, 0);
}
GF_FN float gf_cosf(float y)
{
    const uint32_t t = gf_abstop12(y);
    if (t < 0x3f4) {
        if (GF_UNLIKELY(t < 0x398)) return 1.0f;
        const double x = (double)y;
        return (float)gf_cos_poly(x * x);
    }
    if (GF_UNLIKELY(t >= 0x7f8)) return (y - y) / (y - y);
    return gf_sincos_reduced(y, 1);
}

// ---- asinf (e_asinf.c of glibc 2.35: fdlibm's scheme with a degree-4 polynomial; plain float arithmetic) ----------------------
GF_FN float gf_asinf(float x)
{
    const float pio2_hi = 1.57079637050628662109375f, pio2_lo = -4.37113900018624283e-8f, pio4_hi = 0.785398185253143310546875f;
    const float p0 = 1.666675248e-1f, p1 = 7.495297643e-2f, p2 = 4.547037598e-2f, p3 = 2.417951451e-2f, p4 = 4.216630880e-2f;
    const int32_t hx = (int32_t)gf_asuint(x), ix = hx & 0x7fffffff;
    if (ix == 0x3f800000) return x * pio2_hi + x * pio2_lo;     // asin(+-1) = +-pi/2
    if (ix > 0x3f800000) return (x - x) / (x - x);              // |x| > 1, NaN
    if (ix < 0x3f000000) {                                      // |x| < 0.5
        if (ix < 0x32000000) return x;                          // |x| < 2^-27
        const float t = x * x;
        const float w = t * (p0 + t * (p1 + t * (p2 + t * (p3 + t * p4))));
        return x + x * w;
    }
    float w = 1.0f - __builtin_fabsf(x);
    float t = w * 0.5f;
    float p = t * (p0 + t * (p1 + t * (p2 + t * (p3 + t * p4))));
    const float s = __builtin_sqrtf(t);
    if (ix >= 0x3F79999A) {                                     // |x| > 0.975
        t = pio2_hi - (2.0f * (s + s * p) - pio2_lo);
    } else {
        w = gf_asfloat(gf_asuint(s) & 0xfffff000u);
        const float c = (t - w * w) / (s + w);
        const float r = p;
        p = 2.0f * s * r - (pio2_lo - 2.0f * c);
        const float q = pio4_hi - 2.0f * w;
        t = pio4_hi - (p - q);
    }
    return hx > 0 ? t : -t;
}

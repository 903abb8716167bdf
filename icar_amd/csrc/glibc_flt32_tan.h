// icar_amd/csrc/glibc_flt32_tan.h -- tanf exactly as the compiled reference evaluates it (sibling of glibc_flt32_trig.h, same
// GF_FN / GF_TABLE conventions; nothing of that header is changed, its reduce_large and its 4/pi table are reused).
// Origin and licence: restated from the GNU C Library 2.35 (sysdeps/ieee754/flt-32/s_tanf.c, k_tanf.c: Copyright (C) 1993 Sun
// Microsystems, Inc. (fdlibm): "permission to use, copy, modify, and distribute this software is freely granted, provided that
// this notice is preserved"; the argument reduction of s_sincosf.h: Copyright (C) Free Software Foundation, Inc. / Arm Ltd.),
// GNU Lesser General Public License 2.1 or later.  The algorithms and constants are theirs; this file is a derived work under
// the same terms.
//
// flang lowers REAL(4) tan to tanf (cu_tiedtke.f90's CUENTR_NEW: TAN(3.1415 * r * 0.5) for the organized detrainment of deep
// convection).  What glibc 2.35's tanf is was read off the C library itself, instruction by instruction:
//   * |x| <= 0x3f490fda (~pi/4): fdlibm's __kernel_tanf(x, 0, 1) directly;
//   * above: NOT fdlibm's __ieee754_rem_pio2f / __kernel_rem_pio2f (glibc 2.28 replaced them in s_tanf.c) but the reduction of
//     sinf / cosf in double precision -- reduce_fast below 120, reduce_large (192 bits of 4/pi) above -- whose remainder is split
//     into a REAL(4) head y0 = (float)r and tail y1 = (float)(r - y0) and handed to __kernel_tanf(y0, y1, n even ? 1 : -1);
//   * tanf is not among the functions of which x86-64 glibc selects an FMA build at load time (sinf, cosf, expf, logf, powf
//     are): reduce_fast is a separate multiply and subtract here, where gf_reduce_fast of glibc_flt32_trig.h (sinf's FMA
//     build) contracts them; __kernel_tanf is plain REAL(4) arithmetic with IEEE division.
// No array, no loop: the large-argument path costs three 32 x 32 -> 64 multiplies and needs no scratch memory.
// Checked value by value on all 2^32 arguments against the host's libm (tests/test_glibc_flt32_tanf_host.py; 0 mismatches
// recorded in profiles/r17_steps.md) and on the device (tests/test_gpu_tanf_math.py).
#pragma once
#include "glibc_flt32_trig.h"

// __kernel_tanf (k_tanf.c): tan(x + y) for iy = 1, -1 / tan(x + y) for iy = -1; |x + y| <= pi/4, y the tail of x
GF_FN float gf_kernel_tanf(float x, float y, int iy)
{
    const float pio4 = 7.8539812565e-01f, pio4lo = 3.7748947079e-08f;                       // 0x3f490fda, 0x33222168
    const float T0 = 3.3333334327e-01f, T1 = 1.3333334029e-01f, T2 = 5.3968254477e-02f, T3 = 2.1869488060e-02f, T4 = 8.8632395491e-03f,
                T5 = 3.5920790397e-03f, T6 = 1.4562094584e-03f, T7 = 5.8804126456e-04f, T8 = 2.4646313977e-04f, T9 = 7.8179444245e-05f,
                T10 = 7.1407252108e-05f, T11 = -1.8558637748e-05f, T12 = 2.5907305826e-05f;
    const int32_t hx = (int32_t)gf_asuint(x), ix = hx & 0x7fffffff;
    if (ix < 0x39000000) {                                      // |x| < 2^-13: tan(x) = x, -1 / tan(x) = -1 / x to the last bit
        if ((ix | (iy + 1)) == 0) return 1.0f / __builtin_fabsf(x);
        if (iy == 1) return x;
        return -1.0f / x;
    }
    const bool big = ix >= 0x3f2ca140;                          // |x| >= 0.6744: tan(x) from tan(pi/4 - x)
    if (big) {
        if (hx < 0) { x = -x; y = -y; }
        const float z = pio4 - x;
        const float w = pio4lo - y;
        x = z + w; y = 0.0f;
        if (__builtin_fabsf(x) < 0x1p-13f) return (float)((1 - ((hx >> 30) & 2)) * iy) * (1.0f - (float)(2 * iy) * x);
    }
    float z = x * x;
    float w = z * z;
    // x^5 (T1 + x^2 T2 + ...) as two interleaved chains in x^4
    float r = T1 + w * (T3 + w * (T5 + w * (T7 + w * (T9 + w * T11))));
    float v = z * (T2 + w * (T4 + w * (T6 + w * (T8 + w * (T10 + w * T12)))));
    float s = z * x;
    r = y + z * (s * (r + v) + y);
    r += T0 * s;
    w = x + r;
    if (big) {
        v = (float)iy;
        return (float)(1 - ((hx >> 30) & 2)) * (v - 2.0f * (x - (w * w / (w + v) - r)));
    }
    if (iy == 1) return w;
    // -1 / (x + r) to better than the 2 ulp of a plain division: head and tail of w and of -1 / w
    z = gf_asfloat(gf_asuint(w) & 0xfffff000u);
    v = r - (z - x);                                            // z + v = r + x
    const float a = -1.0f / w;
    const float t = gf_asfloat(gf_asuint(a) & 0xfffff000u);
    s = 1.0f + t * z;
    return t + a * (s + t * v);
}

// reduce_fast (s_sincosf.h) as tanf's build has it: the multiply and the subtraction rounded separately
GF_FN double gf_reduce_fast_nofma(double x, int *np)
{
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const double r = x * hpi_inv;
    const int n = ((int32_t)r + 0x800000) >> 24;
    *np = n;
    return x - (double)n * hpi;
}

GF_FN float gf_tanf(float y)
{
    const uint32_t xi = gf_asuint(y), ix = xi & 0x7fffffffu;
    if (ix <= 0x3f490fda) return gf_kernel_tanf(y, 0.0f, 1);    // |y| ~<= pi/4
    if (GF_UNLIKELY(ix >= 0x7f800000)) return y - y;            // inf, NaN
    double r;
    int n;
    if (gf_abstop12(y) < 0x42f) r = gf_reduce_fast_nofma((double)y, &n);        // abstop12(120.0f)
    else { r = gf_reduce_large(xi, &n); if (xi >> 31) r = -r; }
    const float y0 = (float)r;
    const float y1 = (float)(r - (double)y0);
    return gf_kernel_tanf(y0, y1, 1 - ((n & 1) << 1));
}

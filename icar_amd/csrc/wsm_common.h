// icar_amd/csrc/wsm_common.h -- what WSM3 (mp_wsm3.hip) and WSM6 (mp_wsm6.hip) hold in common, once: only what is the same
// arithmetic in the same order in mp_wsm3.f90 and mp_wsm6.f90.  The slopes are not: slope_wsm3 takes rslopeb through
// exp(log()) and WSM6's slope_rain / _snow / _graup through x**y, as the reference does.
// REAL(4) exp / log / x**y are the C library's expf / logf / powf bit for bit (glibc_flt32.h), sqrt and divide IEEE.
#pragma once
#include "glibc_flt32.h"
#include <cmath>

#define WSM_MAXK 64                 // levels of a column in this build

// module parameters the two schemes share (mp_wsm3.f90:37-56, mp_wsm6.f90:16-43)
#define WSM_dtcldcr 120.f
#define WSM_n0r 8.e6f
#define WSM_avtr 841.9f
#define WSM_bvtr 0.8f
#define WSM_r0 .8e-5f
#define WSM_peaut .55f
#define WSM_xncr 3.e8f
#define WSM_xmyu 1.718e-5f
#define WSM_avts 11.72f
#define WSM_bvts .41f
#define WSM_n0smax 1.e11f
#define WSM_lamdarmax 8.e4f
#define WSM_lamdasmax 1.e5f
#define WSM_dicon 11.9f
#define WSM_dimax 500.e-6f
#define WSM_n0s 2.e6f
#define WSM_alpha .12f
#define WSM_qcrmin 1.e-9f

// what mp_driver.f90:518-550 (WSM6) / :554-585 (WSM3) passes: gravity, cp, cpv, Rd, Rw, 273.15, EP1, EP2, epsilon, XLS, XLV, XLF,
// rhoair0, rhowater, cliq, cice, psat (icar_constants.f90:391-420, wrf_constants.f90:10-67)
struct WsmArgs { float delt, g, cpd, cpv, rd, rv, t0c, ep1, ep2, qmin, xls, xlv0, xlf0, den0, denr, cliq, cice, psat; };

static inline WsmArgs wsm_args(float dt)
{
    WsmArgs A;
    A.delt = dt; A.g = 9.81f; A.cpd = 1012.0f; A.cpv = 4.f * 461.6f; A.rd = 287.058f; A.rv = 461.5f; A.t0c = 273.15f;
    A.ep1 = 461.5f / 287.058f - 1.f; A.ep2 = 287.058f / 461.5f; A.qmin = 1.e-15f; A.xls = 2.85e6f; A.xlv0 = 2.5e6f; A.xlf0 = 3.50e5f;
    A.den0 = 1.28f; A.denr = 1000.f; A.cliq = 4190.f; A.cice = 2106.f; A.psat = 610.78f;
    return A;
}

// minor time steps (mp_wsm3.f90:418-420, mp_wsm6.f90:416-418): their number through *loops, their length returned
static inline float wsm_dtcld(const WsmArgs &A, int *loops)
{
    const long lp = lroundf(A.delt / WSM_dtcldcr);
    *loops = lp > 1 ? (int)lp : 1;
    float dtcld = A.delt / (float)*loops;
    if (A.delt <= WSM_dtcldcr) dtcld = A.delt;
    return dtcld;
}

// rgmma (mp_wsm3.f90:905-922, mp_wsm6.f90:1386-1405): the 10000-term product form of 1/Gamma, host libm like the compiled reference
static inline float wsm_rgmma(float x)
{
    const float euler = 0.577215664901532f;
    if (x == 1.f) return 0.f;
    float r = x * expf(euler * x);
    for (int i = 1; i <= 10000; ++i) { const float y = (float)i; r = r * (1.000f + x / y) * expf(-x / y); }
    return 1.f / r;
}

__device__ __forceinline__ float mx(float a, float b) { return a > b ? a : b; }        // Fortran max / min of two reals
__device__ __forceinline__ float mn(float a, float b) { return a < b ? a : b; }

// saturation coefficients of the inlined fpvs (mp_wsm3.f90:432-441, mp_wsm6.f90:451-461)
struct WsmSat { float ttp, xa, xb, xai, xbi; };
__device__ __forceinline__ WsmSat wsm_sat_coeffs(const WsmArgs &A)
{
    WsmSat S;
    S.ttp = A.t0c + 0.01f;
    const float dldt = A.cpv - A.cliq; S.xa = -dldt / A.rv; S.xb = S.xa + A.xlv0 / (A.rv * S.ttp);
    const float dldti = A.cpv - A.cice; S.xai = -dldti / A.rv; S.xbi = S.xai + A.xls / (A.rv * S.ttp);
    return S;
}

// statement functions diffus, viscos, xka, diffac, venfac (mp_wsm3.f90:376-381, mp_wsm6.f90:384-389); A is the WsmArgs in scope
#define WSM_DIFFUS(x, y) (8.794e-5f * gf_expf(gf_logf(x) * (1.81f)) / (y))
#define WSM_VISCOS(x, y) (1.496e-6f * ((x) * sqrtf(x)) / ((x) + 120.f) / (y))
#define WSM_XKA(x, y) (1.414e3f * WSM_VISCOS(x, y) * (y))
#define WSM_DIFFAC(a, b, c, d, e) ((d) * (a) * (a) / (WSM_XKA(c, d) * A.rv * (c) * (c)) + 1.f / ((e) * WSM_DIFFUS(c, b)))
#define WSM_VENFAC(a, b, c) (gf_expf(gf_logf((WSM_VISCOS(b, c) / WSM_DIFFUS(b, a))) * ((.3333333f))) / sqrtf(WSM_VISCOS(b, c)) * sqrtf(sqrtf(A.den0 / (c))))

// icar_amd/csrc/mp_wsm3.hip -- WSM3 microphysics (Hong, Dudhia, Chen 2004; src/physics/mp_wsm3.f90), SURVEY 8(f) rank 4, behind
// mp()'s dispatch (mp_driver.f90:552-585): wsm32D (:218-903), slope_wsm3 (:1008-1068), wsm3init (:951-1006), statement by statement
// in the reference's operation order; the fall (nislfv_rain_plm) is wsm_fall.h's.  The reference works on (i,k) slabs of one j row;
// nothing couples the columns of a slab.  Everything of wsm32D except the two falls, the melting level and the surface flux is
// level-local, so a minor step runs as: per level at its top (before the first: also the clamps, cpm, xl), one thread per CELL
// (the scheme's exp/log/pow); per column and species the fall; per column the melting level and the surface flux; per level the
// rates, update and condensation.  REAL(4) exp / log / x**y are the C library's expf / logf / powf bit for bit (glibc_flt32.h),
// sqrt and divide IEEE: oracle/wsm3_oracle.c (a separate slab-by-slab restatement of the Fortran, pinned to the compiled
// reference) calls the host's libm, and tests/test_gpu_wsm3.py compares bit for bit.
#include "ctx.h"
#include "wsm_fall.h"
#include <cstring>
#include <cstdlib>

struct wsm3_consts {        // the SAVE variables wsm3init derives, :57-72
    float qc0, qck1, pidnc, bvtr1, bvtr2, bvtr3, bvtr4, g1pbr, g3pbr, g4pbr, g5pbro2, pvtr, eacrr, pacrr, precr1, precr2,
          xmmax, roqimax, bvts1, bvts2, bvts3, bvts4, g1pbs, g3pbs, g4pbs, g5pbso2, pvts, pacrs, precs1, precs2, pidn0r, pidn0s,
          xlv1, pi, rslopermax, rslopesmax, rsloperbmax, rslopesbmax, rsloper2max, rslopes2max, rsloper3max, rslopes3max;
};

// work arrays of one call, all (nx, nz, ny) REAL(4): the level pieces run one thread per CELL (10 M threads at 512x512x40: the
// transcendental-heavy part of the scheme, ~25 exp/log/pow per level), the fall / melt / surface piece one thread per COLUMN
struct Wsm3State {
    wsm3_consts c; bool ready = false;
    float *t = nullptr, *cpm = nullptr, *xl = nullptr, *denfac = nullptr, *qs = nullptr, *rh = nullptr, *vt = nullptr, *denqrs = nullptr,
          *vti = nullptr, *denqci = nullptr, *rain = nullptr, *snow = nullptr, *delq = nullptr, *zi = nullptr;
    size_t n3 = 0;
};

namespace {
// slope_wsm3 (:1008-1068) for ONE level: returns vt, the slopes through the pointers
__device__ inline float wsm3_slope1(const wsm3_consts &C, float qrs, float den, float denfac, float t,
                                    float *rslope, float *rslopeb, float *rslope2, float *rslope3)
{
    const float t0c = 273.15f;
    float pvt;
    if (t >= t0c) {
        pvt = C.pvtr;
        if (qrs <= WSM_qcrmin) {
            *rslope = C.rslopermax; *rslopeb = C.rsloperbmax; *rslope2 = C.rsloper2max; *rslope3 = C.rsloper3max;
        } else {
            *rslope = 1.f / sqrtf(sqrtf(C.pidn0r / (qrs * den)));
            *rslopeb = gf_expf(gf_logf(*rslope) * (WSM_bvtr));
            *rslope2 = *rslope * *rslope;
            *rslope3 = *rslope2 * *rslope;
        }
    } else {
        const float supcol = t0c - t;
        const float n0sfac = mx(mn(gf_expf(WSM_alpha * supcol), WSM_n0smax / WSM_n0s), 1.f);
        pvt = C.pvts;
        if (qrs <= WSM_qcrmin) {
            *rslope = C.rslopesmax; *rslopeb = C.rslopesbmax; *rslope2 = C.rslopes2max; *rslope3 = C.rslopes3max;
        } else {
            *rslope = 1.f / sqrtf(sqrtf(C.pidn0s * n0sfac / (qrs * den)));
            *rslopeb = gf_expf(gf_logf(*rslope) * (WSM_bvts));
            *rslope2 = *rslope * *rslope;
            *rslope3 = *rslope2 * *rslope;
        }
    }
    float vt = pvt * *rslopeb * denfac;
    if (qrs <= 0.0f) vt = 0.0f;
    return vt;
}
struct W3Speed {                    // the refinement of the fall speed: slope_wsm3 of the arrived rain/snow
    const wsm3_consts &C;
    __device__ __forceinline__ float operator()(const float (&q)[1], float den, float denfac, float tk) const
    {
        float r1, r2, r3, r4;
        return wsm3_slope1(C, q[0], den, denfac, tk, &r1, &r2, &r3, &r4);
    }
};

// the statement functions cpmcal, xlcal, conden (:369-382; the other five: wsm_common.h) and the ice number concentration;
// A, C are the arguments in scope
#define W3_CPMCAL(x) (A.cpd * (1.f - mx(x, A.qmin)) + mx(x, A.qmin) * A.cpv)
#define W3_XLCAL(x) (A.xlv0 - C.xlv1 * ((x) - A.t0c))
#define W3_CONDEN(a, b, c, d, e) ((mx(b, A.qmin) - (c)) / (1.f + (d) * (d) / (A.rv * (e)) * (c) / ((a) * (a))))
#define W3_XNI(den_, qci_) mn(mx(5.38e7f * gf_expf(gf_logf(((den_) * mx(qci_, A.qmin))) * (0.75f)), 1.e3f), 1.e6f)

// once per call and level: clamp (:393-398), cpm and xl (:400-405)
__device__ inline void wsm3_level_init(const wsm3_consts &C, const WsmArgs &A, float q, float t, float *qci, float *qrs, float *cpm, float *xl)
{
    *qci = mx(*qci, 0.0f); *qrs = mx(*qrs, 0.0f);
    *cpm = W3_CPMCAL(q); *xl = W3_XLCAL(t);
}

// top of a minor loop, per level (:425-457, :480-484, :506-520): denfac, qs, rh, the terminal velocities and den*q of rain/snow
// and of cloud ice.  (den, qci and t do not change between here and the ice fall, so its velocity is evaluated here.)
__device__ inline void wsm3_level_prep(const wsm3_consts &C, const WsmArgs &A, const WsmSat &S, float t, float q, float qci, float qrs, float den,
                                       float p, float *denfac, float *qs, float *rh, float *vt, float *denqrs, float *vti, float *denqci)
{
    float tv = 1.0f / den;
    tv = tv * A.den0;
    *denfac = sqrtf(tv);
    const float tr = S.ttp / t;
    float qs_;
    if (t < S.ttp) qs_ = A.psat * (gf_expf(gf_logf(tr) * (S.xai))) * gf_expf(S.xbi * (1.f - tr));
    else            qs_ = A.psat * (gf_expf(gf_logf(tr) * (S.xa))) * gf_expf(S.xb * (1.f - tr));
    // qs0 (:450-451) is computed but never used
    qs_ = mn(qs_, 0.99f * p);
    qs_ = A.ep2 * qs_ / (p - qs_);
    qs_ = mx(qs_, A.qmin);
    *qs = qs_;
    *rh = mx(q / qs_, A.qmin);
    float r1, r2, r3, r4;
    *vt = wsm3_slope1(C, qrs, den, *denfac, t, &r1, &r2, &r3, &r4);
    *denqrs = den * qrs;
    if (t < A.t0c && qci > 0.f) {
        const float xmi = den * qci / W3_XNI(den, qci);
        const float diameter = mx(WSM_dicon * sqrtf(xmi), 1.e-25f);
        *vti = 1.49e4f * gf_expf(gf_logf(diameter) * (1.31f));
    } else *vti = 0.f;
    *denqci = den * qci;
}

// melting / freezing at the 0 C level (:532-569) and the surface precipitation (:570-598) of a column, after both falls
__device__ inline void wsm3_melt_surface(const WsmArgs &A, int km, int st, float dtcld, float delqrs, float delqi, float *t, const float *qci, const float *qrs,
                                         const float *w, const float *den, const float *delz, const float *cpm, const float *vt, const float *denqrs,
                                         float *rain, float *rainncv, float *snow, float *snowncv, float *sr)
{
    const float t0c = A.t0c, xlf0 = A.xlf0, denr = A.denr;
    const float fall1 = delqrs / delz[0] / dtcld;                 // fall(i,1); fall(i,k>1) = denqrs*vt/delz is formed where it is read
    const float fallc1 = delqi / delz[0] / dtcld;
    int mstep = 0;
    for (int k = 1; k <= km; ++k) if (t[(k - 1) * st] >= t0c) mstep = k;
    int kwork2 = mstep, kwork1 = mstep;
    if (mstep != 0) { if (w[(mstep - 1) * st] > 0.f) kwork1 = mstep + 1; }
    {
        const int k = kwork1, kk = kwork2;
        if (k * kk >= 1 && k <= km) {
            const int ck = (k - 1) * st, ckk = (kk - 1) * st;
            const float qrsci = qrs[ck] + qci[ck];
            const float fallkk = (kk == 1) ? fall1 : denqrs[ckk] * vt[ckk] / delz[ckk];
            if (qrsci > 0.f || fallkk > 0.f) {
                const float frzmlt = mn(mx(-w[ck] * qrsci / delz[ck], -qrsci / dtcld), qrsci / dtcld);
                const float snomlt = mn(mx(fallkk / den[ckk], -qrs[ck] / dtcld), qrs[ck] / dtcld);
                if (k == kk) t[ck] = t[ck] - xlf0 / cpm[ck] * (frzmlt + snomlt) * dtcld;
                else {
                    t[ck] = t[ck] - xlf0 / cpm[ck] * frzmlt * dtcld;
                    t[ckk] = t[ckk] - xlf0 / cpm[ckk] * snomlt * dtcld;
                }
            }
        }
    }
    float fallsum = fall1, fallsum_qsi = 0.f;
    if ((t0c - t[0]) > 0) { fallsum = fallsum + fallc1; fallsum_qsi = fall1 + fallc1; }
    if (fallsum > 0.f) {
        *rainncv = fallsum * delz[0] / denr * dtcld * 1000.f + *rainncv;
        *rain = fallsum * delz[0] / denr * dtcld * 1000.f + *rain;
    }
    if (fallsum_qsi > 0.f) {
        *snowncv = fallsum_qsi * delz[0] / denr * dtcld * 1000.f + *snowncv;
        *snow = fallsum_qsi * delz[0] / denr * dtcld * 1000.f + *snow;
    }
    if (fallsum > 0.f) *sr = *snowncv / (*rainncv + 1.e-12f);
}

// per level: rates (:599-736), conservation + update (:737-770), condensation (:771-815)
__device__ inline void wsm3_level_rates(const wsm3_consts &C, const WsmArgs &A, const WsmSat &S, float dtcld, float *t_, float *q_, float *qci_, float *qrs_,
                                        float den, float p, float denfac, float qs, float rh, float cpm, float xl)
{
    const float t0c = A.t0c, qmin = A.qmin, xls = A.xls;
    float t = *t_, q = *q_, qci = *qci_, qrs = *qrs_;
    float rslope, rslopeb, rslope2, rslope3;
    (void)wsm3_slope1(C, qrs, den, denfac, t, &rslope, &rslopeb, &rslope2, &rslope3);
    float w1, w2;
    if (t >= t0c) w1 = WSM_DIFFAC(xl, p, t, den, qs);
    else          w1 = WSM_DIFFAC(xls, p, t, den, qs);
    w2 = WSM_VENFAC(p, t, den);
    float pres = 0.f, paut = 0.f, pacr = 0.f, pgen = 0.f, pisd = 0.f, pcon;
    const float supsat = mx(q, qmin) - qs;
    const float satdt = supsat / dtcld;
    if (t >= t0c) {
        // warm rain (:622-645)
        if (qci > C.qc0) {
            paut = C.qck1 * gf_expf(gf_logf(qci) * ((7.f / 3.f)));
            paut = mn(paut, qci / dtcld);
        }
        if (qrs > WSM_qcrmin && qci > qmin) pacr = mn(C.pacrr * rslope3 * rslopeb * qci * denfac, qci / dtcld);
        if (qrs > 0.f) {
            const float coeres = rslope2 * sqrtf(rslope * rslopeb);
            pres = (rh - 1.f) * (C.precr1 * rslope2 + C.precr2 * w2 * coeres) / w1;
            if (pres < 0.f) { pres = mx(pres, -qrs / dtcld); pres = mx(pres, satdt / 2); }
            else pres = mn(pres, satdt / 2);
        }
    } else {
        // cold rain (:646-735)
        const float supcol = t0c - t;
        const float n0sfac = mx(mn(gf_expf(WSM_alpha * supcol), WSM_n0smax / WSM_n0s), 1.f);
        int ifsat = 0;
        const float xni = W3_XNI(den, qci);
        const float eacrs = gf_expf(0.07f * (-supcol));
        if (qrs > WSM_qcrmin && qci > qmin) {
            const float xmi = den * qci / xni;
            const float diameter = mn(WSM_dicon * sqrtf(xmi), WSM_dimax);
            const float vt2i = 1.49e4f * gf_powf(diameter, 1.31f);
            const float vt2s = C.pvts * rslopeb * denfac;
            const float acrfac = 2.f * rslope3 + 2.f * diameter * rslope2 + diameter * diameter * rslope;
            pacr = mn(C.pi * qci * eacrs * WSM_n0s * n0sfac * fabsf(vt2s - vt2i) * acrfac / 4.f, qci / dtcld);
        }
        if (qci > 0.f) {
            const float xmi = den * qci / xni;
            const float diameter = WSM_dicon * sqrtf(xmi);
            pisd = 4.f * diameter * xni * (rh - 1.f) / w1;
            if (pisd < 0.f) { pisd = mx(pisd, satdt / 2); pisd = mx(pisd, -qci / dtcld); }
            else pisd = mn(pisd, satdt / 2);
            if (fabsf(pisd) >= fabsf(satdt)) ifsat = 1;
        }
        if (qrs > 0.f && ifsat != 1) {
            const float coeres = rslope2 * sqrtf(rslope * rslopeb);
            pres = (rh - 1.f) * n0sfac * (C.precs1 * rslope2 + C.precs2 * w2 * coeres) / w1;
            const float supice = satdt - pisd;
            if (pres < 0.f) { pres = mx(pres, -qrs / dtcld); pres = mx(mx(pres, satdt / 2), supice); }
            else pres = mn(mn(pres, satdt / 2), supice);
            if (fabsf(pisd + pres) >= fabsf(satdt)) ifsat = 1;
        }
        if (supsat > 0 && ifsat != 1) {
            const float supice = satdt - pisd - pres;
            const float xni0 = 1.e3f * gf_expf(0.1f * supcol);
            const float roqi0 = 4.92e-11f * gf_expf(gf_logf(xni0) * (1.33f));
            pgen = mx(0.f, (roqi0 / den - mx(qci, 0.f)) / dtcld);
            pgen = mn(mn(pgen, satdt), supice);
        }
        if (qci > 0.f) {
            const float qimax = C.roqimax / den;
            paut = mx(0.f, (qci - qimax) / dtcld);
        }
    }
    // conservation + update (:737-770)
    const float qciik = mx(qmin, qci);
    const float delqci = (paut + pacr - pgen - pisd) * dtcld;
    if (delqci >= qciik) {
        const float facqci = qciik / delqci;
        paut = paut * facqci; pacr = pacr * facqci; pgen = pgen * facqci; pisd = pisd * facqci;
    }
    const float qik = mx(qmin, q);
    const float delq = (pres + pgen + pisd) * dtcld;
    if (delq >= qik) {
        const float facq = qik / delq;
        pres = pres * facq; pgen = pgen * facq; pisd = pisd * facq;
    }
    w2 = -pres - pgen - pisd;
    q = q + w2 * dtcld;
    qci = mx(qci - (paut + pacr - pgen - pisd) * dtcld, 0.f);
    qrs = mx(qrs + (paut + pacr + pres) * dtcld, 0.f);
    if (t < t0c) t = t - xls * w2 / cpm * dtcld;
    else         t = t - xl * w2 / cpm * dtcld;
    // condensation (:781-808)
    const float tr = S.ttp / t;
    float qsw = A.psat * (gf_expf(gf_logf(tr) * (S.xa))) * gf_expf(S.xb * (1.f - tr));
    qsw = mn(qsw, 0.99f * p);
    qsw = A.ep2 * qsw / (p - qsw);
    qsw = mx(qsw, qmin);
    w1 = W3_CONDEN(t, q, qsw, xl, cpm);
    pcon = mn(mx(w1, 0.f), mx(q, 0.f)) / dtcld;
    if (qci > 0.f && w1 < 0.f && t > t0c) pcon = mx(w1, -qci) / dtcld;
    q = q - pcon * dtcld;
    qci = mx(qci + pcon * dtcld, 0.f);
    t = t + pcon * xl / cpm * dtcld;
    if (qci <= qmin) qci = 0.0f;                                                                          // :809-815
    if (qrs <= WSM_qcrmin) qrs = 0.0f;
    *t_ = t; *q_ = q; *qci_ = qci; *qrs_ = qrs;
}

// wsm3init (:951-1006) with the arguments of mp_driver.f90:105: REAL(4) arithmetic in the reference's order, libm for
// exp / atan / x**y (host side, once)
void wsm3_init_consts(wsm3_consts &C, float den0, float denr, float dens, float cl, float cpv)
{
    C.pi = 4.f * atanf(1.f);
    C.xlv1 = cl - cpv;
    C.qc0 = 4.f / 3.f * C.pi * denr * (WSM_r0 * WSM_r0 * WSM_r0) * WSM_xncr / den0;
    C.qck1 = .104f * 9.8f * WSM_peaut / powf(WSM_xncr * denr, 1.f / 3.f) / WSM_xmyu * powf(den0, 4.f / 3.f);
    C.pidnc = C.pi * denr / 6.f;
    C.bvtr1 = 1.f + WSM_bvtr; C.bvtr2 = 2.5f + .5f * WSM_bvtr; C.bvtr3 = 3.f + WSM_bvtr; C.bvtr4 = 4.f + WSM_bvtr;
    C.g1pbr = wsm_rgmma(C.bvtr1); C.g3pbr = wsm_rgmma(C.bvtr3); C.g4pbr = wsm_rgmma(C.bvtr4); C.g5pbro2 = wsm_rgmma(C.bvtr2);
    C.pvtr = WSM_avtr * C.g4pbr / 6.f;
    C.eacrr = 1.0f;
    C.pacrr = C.pi * WSM_n0r * WSM_avtr * C.g3pbr * .25f * C.eacrr;
    C.precr1 = 2.f * C.pi * WSM_n0r * .78f;
    C.precr2 = 2.f * C.pi * WSM_n0r * .31f * powf(WSM_avtr, .5f) * C.g5pbro2;
    C.xmmax = (WSM_dimax / WSM_dicon) * (WSM_dimax / WSM_dicon);
    { const float d2 = WSM_dimax * WSM_dimax, d4 = d2 * d2; C.roqimax = 2.08e22f * (d4 * d4); }
    C.bvts1 = 1.f + WSM_bvts; C.bvts2 = 2.5f + .5f * WSM_bvts; C.bvts3 = 3.f + WSM_bvts; C.bvts4 = 4.f + WSM_bvts;
    C.g1pbs = wsm_rgmma(C.bvts1); C.g3pbs = wsm_rgmma(C.bvts3); C.g4pbs = wsm_rgmma(C.bvts4); C.g5pbso2 = wsm_rgmma(C.bvts2);
    C.pvts = WSM_avts * C.g4pbs / 6.f;
    C.pacrs = C.pi * WSM_n0s * WSM_avts * C.g3pbs * .25f;
    C.precs1 = 4.f * WSM_n0s * .65f;
    C.precs2 = 4.f * WSM_n0s * .44f * powf(WSM_avts, .5f) * C.g5pbso2;
    C.pidn0r = C.pi * denr * WSM_n0r;
    C.pidn0s = C.pi * dens * WSM_n0s;
    C.rslopermax = 1.f / WSM_lamdarmax; C.rslopesmax = 1.f / WSM_lamdasmax;
    C.rsloperbmax = powf(C.rslopermax, WSM_bvtr); C.rslopesbmax = powf(C.rslopesmax, WSM_bvts);
    C.rsloper2max = C.rslopermax * C.rslopermax; C.rslopes2max = C.rslopesmax * C.rslopesmax;
    C.rsloper3max = C.rsloper2max * C.rslopermax; C.rslopes3max = C.rslopes2max * C.rslopesmax;
}
struct W3Work { float *t, *cpm, *xl, *denfac, *qs, *rh, *vt, *denqrs, *vti, *denqci, *rain, *snow, *zi; };

// once per call and column: the interface heights the wave falls read
__global__ void __launch_bounds__(64)
k_wsm3_zi(Dims d, const float *__restrict__ delz, float *__restrict__ zi, int i0, int i1, int j0, int k0, int km)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y;
    if (i > i1) return;
    wsm_zi_column(d, delz, zi, i, j, k0, km);
}

// per cell, top of a minor loop (first: also t = th*pii (:151-155), the clamps, cpm, xl)
template <bool FIRST>
__global__ void __launch_bounds__(256)
k_wsm3_prep(Dims d, wsm3_consts C, WsmArgs A, W3Work W, const float *__restrict__ th, const float *__restrict__ pii, const float *__restrict__ q,
            float *__restrict__ qci, float *__restrict__ qrs, const float *__restrict__ den, const float *__restrict__ p,
            int i0, int i1, int j0, int k0, int km)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, k = k0 + blockIdx.y * 4 + threadIdx.y, j = j0 + blockIdx.z;
    if (i > i1 || k - k0 >= km) return;
    const int c = d.idx(i, k, j);
    const WsmSat S = wsm_sat_coeffs(A);
    float t, qci_ = qci[c], qrs_ = qrs[c];
    if (FIRST) {
        if (k == k0) { const int c2 = i + d.nx * j; W.rain[c2] = 0.f; W.snow[c2] = 0.f; }      // process_subdomain: precipitation = 0, snowfall = 0
        t = th[c] * pii[c];
        float cpm, xl;
        wsm3_level_init(C, A, q[c], t, &qci_, &qrs_, &cpm, &xl);
        W.t[c] = t; W.cpm[c] = cpm; W.xl[c] = xl; qci[c] = qci_; qrs[c] = qrs_;
    } else t = W.t[c];
    float denfac, qs, rh, vt, denqrs, vti, denqci;
    wsm3_level_prep(C, A, S, t, q[c], qci_, qrs_, den[c], p[c], &denfac, &qs, &rh, &vt, &denqrs, &vti, &denqci);
    W.denfac[c] = denfac; W.qs[c] = qs; W.rh[c] = rh; W.vt[c] = vt; W.denqrs[c] = denqrs; W.vti[c] = vti; W.denqci[c] = denqci;
}


// The falls with lane = level (wsm_fall.h's wave form).  A block = 4 waves = one row segment of W3_TC columns of one species: the
// seven column arrays are staged through LDS as [level][column] tiles (coalesced 128-B row reads; the column-per-wave access
// pattern itself would touch one cache line per lane), each wave then walks its W3_TC/4 columns with lane = level, and the
// results go back the same way.
#define W3_TC 16      // (16 columns = 15 kB of LDS per block: more blocks per CU than with 32; measured with mp_wsm6.hip's falls)
__global__ void __launch_bounds__(256)
k_wsm3_fall_tile(Dims d, wsm3_consts C, W3Work W, float *__restrict__ qci, float *__restrict__ qrs, const float *__restrict__ den_,
                 const float *__restrict__ delz, float *__restrict__ delq, float dt, int i0, int i1, int j0, int k0, int km)
{
    extern __shared__ float w3_lds[];                                // [7][km][W3_TC + 1]
    const int ib = i0 + blockIdx.x * W3_TC, j = j0 + blockIdx.y;
    const bool ice = blockIdx.z == 1;
    const int ncol = min(W3_TC, i1 - ib + 1);
    const int LS = W3_TC + 1, plane = km * LS;
    float *__restrict__ qx = ice ? qci : qrs;
    float *__restrict__ denq = ice ? W.denqci : W.denqrs;
    const float *src[7] = {delz, den_, W.denfac, W.t, ice ? W.vti : W.vt, denq, W.zi};
    for (int a = 0; a < 7; ++a)
        for (int e = threadIdx.x; e < km * W3_TC; e += 256) {
            const int k = e / W3_TC, ci = e % W3_TC;
            if (ci < ncol) w3_lds[a * plane + k * LS + ci] = src[a][d.idx(ib + ci, k0 + k, j)];
        }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane < km ? lane : km - 1;                        // lanes beyond the column read a valid level (values unused)
    for (int t = 0; t < W3_TC / 4; ++t) {
        const int ci = wave * (W3_TC / 4) + t;
        if (ci >= ncol) break;                                       // wave-uniform
        const float dz = w3_lds[0 * plane + kl * LS + ci], den = w3_lds[1 * plane + kl * LS + ci], denfac = w3_lds[2 * plane + kl * LS + ci],
                    tk = w3_lds[3 * plane + kl * LS + ci], wwl = w3_lds[4 * plane + kl * LS + ci];
        const float rql[1] = {w3_lds[5 * plane + kl * LS + ci]};
        const int kz = (lane <= km ? lane : km) - 1;
        const float zi = lane == 0 ? 0.0f : w3_lds[6 * plane + kz * LS + ci];
        float qn[1], precip[1];
        wsm_fall_wave<1>(km, lane, dz, den, denfac, tk, wwl, rql, zi, dt, ice ? 0 : 1, W3Speed{C}, qn, precip);   // :521-528 iter = 0, :485-498 iter = 1
        if (lane < km) w3_lds[5 * plane + lane * LS + ci] = qn[0];   // this wave is the only reader / writer of column ci
        if (lane == 0) delq[(size_t)(ice ? 1 : 0) * d.nx * d.ny + (ib + ci) + d.nx * j] = precip[0];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < km * W3_TC; e += 256) {
        const int k = e / W3_TC, ci = e % W3_TC;
        if (ci < ncol) {
            const int c = d.idx(ib + ci, k0 + k, j);
            const float qn = w3_lds[5 * plane + k * LS + ci];
            denq[c] = qn;                                            // rql(i,:) = qn(:)
            qx[c] = mx(qn / w3_lds[1 * plane + k * LS + ci], 0.f);   // q = max(den*q / den, 0)
        }
    }
}

// per column and species (blockIdx.z: 0 rain/snow :485-498 with iter = 1, 1 cloud ice :521-528 with iter = 0), for columns too tall
// for a wave: the serial fall on den*q, then q = max(den*q / den, 0).  The column arrays are read and written in place (element
// stride nx, coalesced across the lanes of a wave); only the fall's work arrays are private.  The two species are independent
// until the melting level, which doubles the number of (serial) threads.
__global__ void __launch_bounds__(64)
k_wsm3_fall(Dims d, wsm3_consts C, W3Work W, float *__restrict__ qci, float *__restrict__ qrs, const float *__restrict__ den,
            const float *__restrict__ delz, float *__restrict__ delq, float dtcld, int i0, int i1, int j0, int k0, int km)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y;
    if (i > i1) return;
    const int c0 = d.idx(i, k0, j), c2 = i + d.nx * j, st = d.sk;
    const bool ice = blockIdx.z == 1;
    float *const qx = (ice ? qci : qrs) + c0, *const denq[1] = {(ice ? W.denqci : W.denqrs) + c0};
    float precip[1];
    wsm_fall_column<1>(km, st, den + c0, W.denfac + c0, W.t + c0, delz + c0, (ice ? W.vti : W.vt) + c0, denq, dtcld, ice ? 0 : 1, W3Speed{C}, precip);
    for (int k = 0; k < km; ++k) qx[k * st] = mx(denq[0][k * st] / den[c0 + k * st], 0.f);
    delq[(size_t)blockIdx.z * d.nx * d.ny + c2] = precip[0];
}

// per column: melting level and surface flux (this call's REAL(4) sums in W.rain / W.snow)
__global__ void __launch_bounds__(64)
k_wsm3_melt(Dims d, WsmArgs A, W3Work W, const float *__restrict__ qci, const float *__restrict__ qrs, const float *__restrict__ w,
            const float *__restrict__ den, const float *__restrict__ delz, const float *__restrict__ delq, float dtcld,
            int i0, int i1, int j0, int k0, int km)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y;
    if (i > i1) return;
    const int c0 = d.idx(i, k0, j), c2 = i + d.nx * j;
    float rain = W.rain[c2], snow = W.snow[c2], rainncv = 0.f, snowncv = 0.f, sr = 0.f;   // rainncv / snowncv / sr only feed sr, which ICAR drops
    wsm3_melt_surface(A, km, d.sk, dtcld, delq[c2], delq[(size_t)d.nx * d.ny + c2], W.t + c0, qci + c0, qrs + c0, w + c0, den + c0, delz + c0,
                      W.cpm + c0, W.vt + c0, W.denqrs + c0, &rain, &rainncv, &snow, &snowncv, &sr);
    W.rain[c2] = rain; W.snow[c2] = snow;
}

// per cell: rates, update, condensation; LAST: th = t / pii (:171-175)
template <bool LAST>
__global__ void __launch_bounds__(256)
k_wsm3_rates(Dims d, wsm3_consts C, WsmArgs A, W3Work W, float *__restrict__ th, const float *__restrict__ pii, float *__restrict__ q,
             float *__restrict__ qci, float *__restrict__ qrs, const float *__restrict__ den, const float *__restrict__ p, float dtcld,
             int i0, int i1, int j0, int k0, int km)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, k = k0 + blockIdx.y * 4 + threadIdx.y, j = j0 + blockIdx.z;
    if (i > i1 || k - k0 >= km) return;
    const int c = d.idx(i, k, j);
    const WsmSat S = wsm_sat_coeffs(A);
    float t = W.t[c], q_ = q[c], qci_ = qci[c], qrs_ = qrs[c];
    wsm3_level_rates(C, A, S, dtcld, &t, &q_, &qci_, &qrs_, den[c], p[c], W.denfac[c], W.qs[c], W.rh[c], W.cpm[c], W.xl[c]);
    q[c] = q_; qci[c] = qci_; qrs[c] = qrs_;
    if (LAST) th[c] = t / pii[c]; else W.t[c] = t;
}

// mp_driver.f90:587-595: REAL(8) accumulators += this call's REAL(4) precipitation / snowfall
__global__ void k_wsm3_accumulate(Dims d, W3Work W, double *__restrict__ precip_acc, double *__restrict__ snow_acc, int i0, int i1, int j0)
{
    const int i = i0 + blockIdx.x * 64 + threadIdx.x, j = j0 + blockIdx.y;
    if (i > i1) return;
    const int c2 = i + d.nx * j;
    precip_acc[c2] = precip_acc[c2] + W.rain[c2];
    snow_acc[c2] = snow_acc[c2] + W.snow[c2];
}
}  // namespace

void icar_wsm3_free(icar_hip_ctx *c)
{
    if (!c->wsm3) return;
    float **ps[] = {&c->wsm3->t, &c->wsm3->cpm, &c->wsm3->xl, &c->wsm3->denfac, &c->wsm3->qs, &c->wsm3->rh, &c->wsm3->vt, &c->wsm3->denqrs,
                    &c->wsm3->vti, &c->wsm3->denqci, &c->wsm3->rain, &c->wsm3->snow, &c->wsm3->delq, &c->wsm3->zi};
    for (float **p : ps) if (*p) hipFree(*p);
    delete c->wsm3; c->wsm3 = nullptr;
}

int icar_wsm3_init_run(icar_hip_ctx *c)
{
    // wsm3init(rhoair0, rhowater, rhosnow, cliq, cpv) as mp_driver.f90:105 calls it (wrf_constants.f90:30-35, :65-67)
    if (!c->wsm3) c->wsm3 = new Wsm3State;
    wsm3_init_consts(c->wsm3->c, 1.28f, 1000.f, 100.f, 4190.f, 4.f * 461.6f);
    c->wsm3->ready = true;
    return 0;
}

int icar_wsm3_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    if (!c->wsm3 || !c->wsm3->ready) { icar_set_error("wsm3: call icar_hip_wsm3_init first"); return 1; }
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme || kts < c->kms || kte > c->kme) { icar_set_error("wsm3: tile outside memory bounds"); return 1; }
    if (ite < its || jte < jts) return 0;
    const int km = kte - kts + 1;
    if (km < 3 || km > WSM_MAXK) { icar_set_error("wsm3: 3..64 levels in this build"); return 1; }
    float *th = icar_field_f(c, ICAR_F_POTENTIAL_TEMPERATURE), *q = icar_field_f(c, ICAR_F_WATER_VAPOR);
    float *qci = icar_field_f(c, ICAR_F_CLOUD_WATER), *qrs = icar_field_f(c, ICAR_F_RAIN);
    const float *w = icar_field_f(c, ICAR_F_W_REAL), *den = icar_field_f(c, ICAR_F_DENSITY), *pii = icar_field_f(c, ICAR_F_EXNER);
    const float *p = icar_field_f(c, ICAR_F_PRESSURE), *dz = icar_field_f(c, ICAR_F_DZ_MASS);
    double *pa = (double *)icar_field_f(c, ICAR_F_PRECIPITATION, false), *sa = (double *)icar_field_f(c, ICAR_F_SNOWFALL, false);
    if (!th || !q || !qci || !qrs || !w || !den || !pii || !p || !dz || !pa || !sa) return 1;
    Wsm3State *S = c->wsm3;
    if (!S->t) {
        float **p3[] = {&S->t, &S->cpm, &S->xl, &S->denfac, &S->qs, &S->rh, &S->vt, &S->denqrs, &S->vti, &S->denqci, &S->zi};
        for (float **x : p3) HIPCHK(hipMalloc(x, c->n3 * sizeof(float)));
        HIPCHK(hipMalloc(&S->rain, (size_t)c->d.nx * c->d.ny * sizeof(float))); HIPCHK(hipMalloc(&S->snow, (size_t)c->d.nx * c->d.ny * sizeof(float)));
        HIPCHK(hipMalloc(&S->delq, 2 * (size_t)c->d.nx * c->d.ny * sizeof(float)));
    }
    const WsmArgs A = wsm_args(dt);
    int loops; const float dtcld = wsm_dtcld(A, &loops);
    W3Work W = {S->t, S->cpm, S->xl, S->denfac, S->qs, S->rh, S->vt, S->denqrs, S->vti, S->denqci, S->rain, S->snow, S->zi};
    ScopedTimer tm(c, "mp");
    // (the call's REAL(4) surface sums are zeroed per column by k_wsm3_prep: calls on disjoint tiles -- the strips and the interior on
    // the context's two streams -- share no scratch)
    const int i0 = its - c->ims, i1 = ite - c->ims, j0 = jts - c->jms, k0 = kts - c->kms, nxb = (ite - its + 1 + 63) / 64, nyt = jte - jts + 1;
    const dim3 gc(nxb, (km + 3) / 4, nyt), bc(64, 4), g2(nxb, nyt), b2(64);
    hipLaunchKernelGGL(k_wsm3_zi, g2, b2, 0, c->stream, c->d, dz, S->zi, i0, i1, j0, k0, km);
    for (int loop = 1; loop <= loops; ++loop) {
        if (loop == 1) hipLaunchKernelGGL((k_wsm3_prep<true>), gc, bc, 0, c->stream, c->d, S->c, A, W, th, pii, q, qci, qrs, den, p, i0, i1, j0, k0, km);
        else           hipLaunchKernelGGL((k_wsm3_prep<false>), gc, bc, 0, c->stream, c->d, S->c, A, W, th, pii, q, qci, qrs, den, p, i0, i1, j0, k0, km);
        if (km + 1 <= 64) {                                   // lane = level; more levels: one thread per column
            const int ncol_x = ite - its + 1;
            hipLaunchKernelGGL(k_wsm3_fall_tile, dim3((ncol_x + W3_TC - 1) / W3_TC, nyt, 2), dim3(256), 7 * (size_t)km * (W3_TC + 1) * sizeof(float),
                               c->stream, c->d, S->c, W, qci, qrs, den, dz, S->delq, dtcld, i0, i1, j0, k0, km);
        } else
            hipLaunchKernelGGL(k_wsm3_fall, dim3(nxb, nyt, 2), b2, 0, c->stream, c->d, S->c, W, qci, qrs, den, dz, S->delq, dtcld, i0, i1, j0, k0, km);
        hipLaunchKernelGGL(k_wsm3_melt, g2, b2, 0, c->stream, c->d, A, W, qci, qrs, w, den, dz, S->delq, dtcld, i0, i1, j0, k0, km);
        if (loop == loops) hipLaunchKernelGGL((k_wsm3_rates<true>), gc, bc, 0, c->stream, c->d, S->c, A, W, th, pii, q, qci, qrs, den, p, dtcld, i0, i1, j0, k0, km);
        else               hipLaunchKernelGGL((k_wsm3_rates<false>), gc, bc, 0, c->stream, c->d, S->c, A, W, th, pii, q, qci, qrs, den, p, dtcld, i0, i1, j0, k0, km);
    }
    hipLaunchKernelGGL(k_wsm3_accumulate, g2, b2, 0, c->stream, c->d, W, pa, sa, i0, i1, j0);
    HIPCHK(hipGetLastError());
    return 0;
}

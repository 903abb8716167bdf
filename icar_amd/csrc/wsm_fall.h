// icar_amd/csrc/wsm_fall.h -- the semi-Lagrangian fall with a piecewise-linear reconstruction that WSM3 and WSM6 sediment with:
// nislfv_rain_plm (mp_wsm3.f90:1266-1505, mp_wsm6.f90:1723-1961) and its two-field variant nislfv_rain_plm6 (mp_wsm6.f90:1963-2230),
// once per form.  The serial form (one thread per column) serves columns of more than 63 levels, the wave form (one wave per
// column, lane = level) all others.  Both take NF fields of den*q that fall with ONE speed (1, or WSM6's snow + graupel: one
// arrival computation, two remaps) and a callable
//     speed(q[NF], den, denfac, tk) -> terminal velocity of a level from the arrived mixing ratios
// that the one refinement of the speed (iter = 1) calls; iter = 0 (cloud ice) never calls it.  The reference's scratch copies
// qq (= rql), wd (= wwl) and the unused slope outputs of its iteration are not materialised.
#pragma once
#include "ctx.h"
#include "wsm_common.h"

namespace {

// zi(k+1) = zi(k) + dz(k) (mp_wsm3.f90:1291-1294), the reference's running sum, of column (i, j): once per call
__device__ __forceinline__ void wsm_zi_column(const Dims &d, const float *__restrict__ delz, float *__restrict__ zi, int i, int j, int k0, int km)
{
    float run = 0.0f;
    for (int k = 0; k < km; ++k) { const int c = d.idx(i, k0 + k, j); run = run + delz[c]; zi[c] = run; }
}

// ---------------- serial form: one thread per column ----------------
// Column arrays are addressed with the element stride st (level k of a column is k*st away in the (i,k,j) fields).
struct WsmFallGeom { float zi[WSM_MAXK + 1], za[WSM_MAXK + 1], dza[WSM_MAXK + 1]; };

// interface speeds (third-order interpolation; the linear estimate before it is overwritten), rain-shaft top, the 5 % deformation
// limiter, and the arrival heights
__device__ void wsm_arrival(int km, int st, const float *ww, const float *__restrict__ dz, float dt, WsmFallGeom &G)
{
    float wi[WSM_MAXK + 1];
    const float fa1 = 9.f / 16.f, fa2 = 1.f / 16.f, con1 = 0.05f;
    wi[0] = ww[0];
    wi[1] = 0.5f * (ww[1] + ww[0]);
    for (int k = 2; k < km - 1; ++k) wi[k] = fa1 * (ww[k] + ww[k - 1]) - fa2 * (ww[k + 1] + ww[k - 2]);
    wi[km - 1] = 0.5f * (ww[km - 1] + ww[km - 2]);
    wi[km] = ww[km - 1];
    for (int k = 1; k < km; ++k) if (ww[k] == 0.0f) wi[k] = ww[k - 1];
    for (int k = km - 1; k >= 0; --k) {
        const float dzk = dz[k * st];
        const float decfl = (wi[k + 1] - wi[k]) * dt / dzk;
        if (decfl > con1) wi[k] = wi[k + 1] - con1 * dzk / dt;
    }
    for (int k = 0; k <= km; ++k) G.za[k] = G.zi[k] - wi[k] * dt;
    for (int k = 0; k < km; ++k) G.dza[k] = G.za[k + 1] - G.za[k];
    G.dza[km] = G.zi[km] - G.za[km];
}

// piecewise-linear reconstruction of qa on the arrival grid, remap onto the regular levels (written to out, stride st), and the
// part that left through the ground (returned)
__device__ float wsm_remap(int km, int st, const WsmFallGeom &G, const float *qa, float *__restrict__ out)
{
    float qmi[WSM_MAXK + 1], qpi[WSM_MAXK + 1];
    const float *zi = G.zi, *za = G.za, *dza = G.dza;
    for (int k = 1; k < km; ++k) {
        const float dip = (qa[k + 1] - qa[k]) / (dza[k + 1] + dza[k]);
        const float dim = (qa[k] - qa[k - 1]) / (dza[k - 1] + dza[k]);
        if (dip * dim <= 0.0f) { qmi[k] = qa[k]; qpi[k] = qa[k]; }
        else {
            qpi[k] = qa[k] + 0.5f * (dip + dim) * dza[k];
            qmi[k] = 2.0f * qa[k] - qpi[k];
            if (qpi[k] < 0.0f || qmi[k] < 0.0f) { qpi[k] = qa[k]; qmi[k] = qa[k]; }
        }
    }
    qpi[0] = qa[0]; qmi[0] = qa[0]; qmi[km] = qa[km]; qpi[km] = qa[km];
    int kb = 1, kt = 1, k = 1;                               // 1-based like the reference's; levels the loop leaves early stay 0
    for (; k <= km; ++k) {
        kb = kb - 1 > 1 ? kb - 1 : 1;
        kt = kt - 1 > 1 ? kt - 1 : 1;
        if (zi[k - 1] >= za[km]) break;
        for (int kk = kb; kk <= km; ++kk) if (zi[k - 1] <= za[kk]) { kb = kk; break; }
        for (int kk = kt; kk <= km; ++kk) if (zi[k] <= za[kk - 1]) { kt = kk; break; }
        kt = kt - 1;
        float qn = 0.0f;
        if (kt == kb) {
            const float tl = (zi[k - 1] - za[kb - 1]) / dza[kb - 1];
            const float th = (zi[k] - za[kb - 1]) / dza[kb - 1];
            const float tl2 = tl * tl, th2 = th * th;
            const float qqd = 0.5f * (qpi[kb - 1] - qmi[kb - 1]);
            const float qqh = qqd * th2 + qmi[kb - 1] * th;
            const float qql = qqd * tl2 + qmi[kb - 1] * tl;
            qn = (qqh - qql) / (th - tl);
        } else if (kt > kb) {
            const float tl = (zi[k - 1] - za[kb - 1]) / dza[kb - 1];
            const float tl2 = tl * tl;
            float qqd = 0.5f * (qpi[kb - 1] - qmi[kb - 1]);
            const float qql = qqd * tl2 + qmi[kb - 1] * tl;
            const float dql = qa[kb - 1] - qql;
            float zsum = (1.f - tl) * dza[kb - 1];
            float qsum = dql * dza[kb - 1];
            for (int m = kb + 1; m <= kt - 1; ++m) { zsum = zsum + dza[m - 1]; qsum = qsum + qa[m - 1] * dza[m - 1]; }
            const float th = (zi[k] - za[kt - 1]) / dza[kt - 1];
            const float th2 = th * th;
            qqd = 0.5f * (qpi[kt - 1] - qmi[kt - 1]);
            const float dqh = qqd * th2 + qmi[kt - 1] * th;
            zsum = zsum + th * dza[kt - 1];
            qsum = qsum + dqh * dza[kt - 1];
            qn = qsum / zsum;
        }
        out[(k - 1) * st] = qn;
    }
    for (; k <= km; ++k) out[(k - 1) * st] = 0.0f;
    float precip = 0.0f;
    for (int kk = 0; kk < km; ++kk) {
        if (za[kk] < 0.0f && za[kk + 1] < 0.0f) { precip = precip + qa[kk] * dza[kk]; continue; }
        else if (za[kk] < 0.0f && za[kk + 1] >= 0.0f) { precip = precip + qa[kk] * (0.0f - za[kk]); break; }
        break;
    }
    return precip;
}

// one column: rql[f] hold den*q on input and output, wwl the terminal velocity (a local copy is refined; the caller's array is
// not changed, as in the reference), precip[f] = what left through the ground
template <int NF, class Speed>
__device__ void wsm_fall_column(int km, int st, const float *__restrict__ den, const float *__restrict__ denfac, const float *__restrict__ tk,
                                const float *__restrict__ dz, const float *__restrict__ wwl, float *const *rql, float dt, int iter, Speed speed,
                                float *precip)
{
    WsmFallGeom G;
    float ww[WSM_MAXK], qa[NF][WSM_MAXK + 1];
    for (int f = 0; f < NF; ++f) precip[f] = 0.0f;
    float allold = 0.0f;
    for (int k = 0; k < km; ++k) {
        ww[k] = wwl[k * st];
        for (int f = 0; f < NF; ++f) allold = allold + rql[f][k * st];
    }
    if (allold <= 0.0f) return;                              // cycle i_loop: the column keeps its den*q
    G.zi[0] = 0.0f;
    for (int k = 0; k < km; ++k) G.zi[k + 1] = G.zi[k] + dz[k * st];
    for (int n = 1;; ++n) {
        wsm_arrival(km, st, ww, dz, dt, G);
        for (int k = 0; k < km; ++k)
            for (int f = 0; f < NF; ++f) qa[f][k] = rql[f][k * st] * dz[k * st] / G.dza[k];
        for (int f = 0; f < NF; ++f) qa[f][km] = 0.0f;
        if (n > iter) break;
        for (int k = 0; k < km; ++k) {                       // one refinement of the speed with the arrived mixing ratios
            const float dk = den[k * st];
            float q[NF];
            for (int f = 0; f < NF; ++f) q[f] = qa[f][k] / dk;
            ww[k] = 0.5f * (wwl[k * st] + speed(q, dk, denfac[k * st], tk[k * st]));
        }
    }
    for (int f = 0; f < NF; ++f) precip[f] = wsm_remap(km, st, G, qa[f], rql[f]);
}

// ---------------- wave form: one WAVE per column, lane = level (cell quantities) / interface (wi, zi, za, dza, qa, qmi, qpi live
// on lanes 0..km).  nislfv_rain_plm is sequential in k only in four places, which stay sequential here so that every sum and
// every comparison sees the reference's operands:
//   zi            running sum of dz: a field filled once per call (wsm_zi_column)
//   wi limiter    k = km..1 uses the wi(k+1) it may just have changed: evaluated for all k at once with the unmodified values;
//                 only from the highest level that trips the limit downward is it re-run serially (rare)
//   kb / kt       "first kk >= previous-1 with zi <= za(kk)": za is strictly increasing (the limiter guarantees dza >= 0.95 dz),
//                 so the first kk is the count of arrival heights below zi, the same for every start the reference can have;
//                 where kt is not found the reference's stale kt is < kb and the level gets qn = 0 either way
//   sums          the kb+1..kt-1 partial sums and the surface flux are short loops in k order
// Needs km + 1 <= 64 lanes; all cross-lane reads happen with every lane active.
// Nearest-neighbour lane reads are DPP wave shifts (v_mov_b32_dpp wave_shr:1 / wave_shl:1: one VALU slot; __shfl_up / __shfl_down are
// ds_bpermute_b32 at 24 cycles per wave, profiles/micro/valubench.hip).  A lane without a source reads 0; none of those values is used.
__device__ __forceinline__ float wsm_up(float x)     // value of lane-1 (0 in lane 0)
{ return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x138, 0xf, 0xf, true)); }
__device__ __forceinline__ float wsm_dn(float x)     // value of lane+1 (0 in lane 63)
{ return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x130, 0xf, 0xf, true)); }

// interface speeds, limiter, arrival heights: ww per cell lane -> za, dza per interface lane
__device__ __forceinline__ void wsm_wave_arrival(int km, int lane, float ww, float dz, float zi, float dt, float &za, float &dza)
{
    const bool cell = lane < km;
    const float wm1 = wsm_up(ww), wm2 = wsm_up(wm1), wp1 = wsm_dn(ww);
    const float fa1 = 9.f / 16.f, fa2 = 1.f / 16.f, con1 = 0.05f;
    float wi;
    if (lane == 0) wi = ww;
    else if (lane == 1) wi = 0.5f * (ww + wm1);
    else if (lane <= km - 2) wi = fa1 * (ww + wm1) - fa2 * (wp1 + wm2);
    else if (lane == km - 1) wi = 0.5f * (ww + wm1);
    else wi = wm1;                                           // lane == km: wi(km+1) = ww(km)
    if (lane >= 1 && lane < km && ww == 0.0f) wi = wm1;      // terminate at the top of the rain shaft
    const float wip1 = wsm_dn(wi);
    const float dec = (wip1 - wi) * dt / dz;
    const unsigned long long bad = __ballot(cell && dec > con1);
    if (bad) {                                               // wave-uniform
        // Serial only where it has to be: level k must be re-evaluated when wi(k+1) has just been changed; when a level is left
        // alone, everything below it still sees the values the parallel evaluation saw, so the walk jumps to the next level
        // that tripped there.
        const float cdz = con1 * dz / dt;                    // per lane, the reference's con1*dz(k)/dt
        unsigned long long rem = bad;
        int k = 63 - __builtin_clzll(rem);
        while (k >= 0) {
            const float wk1 = __shfl(wi, k + 1), wk = __shfl(wi, k), dzk = __shfl(dz, k), ck = __shfl(cdz, k);
            const float decfl = (wk1 - wk) * dt / dzk;
            rem &= (k == 0) ? 0ull : ((1ull << k) - 1ull);   // levels below k that tripped with the unmodified values
            if (decfl > con1) { if (lane == k) wi = wk1 - ck; k = k - 1; }   // uniform: all lanes hold the same broadcast operands
            else k = rem ? 63 - __builtin_clzll(rem) : -1;
        }
    }
    za = zi - wi * dt;                                       // interfaces 0..km
    const float zap1 = wsm_dn(za);
    dza = (lane < km) ? zap1 - za : zi - za;                 // dza(km+1) = zi(km+1) - za(km+1)
}

// reconstruction, remap and rain-out of one arrived field: returns this lane's qn, adds to precip
__device__ __forceinline__ float wsm_wave_remap(int km, int lane, float zi, float za, float dza, float qa, float &precip)
{
    const bool cell = lane < km;
    float qmi = qa, qpi = qa;                                // piecewise-linear reconstruction
    {
        const float qap1 = wsm_dn(qa), qam1 = wsm_up(qa), dzap1 = wsm_dn(dza), dzam1 = wsm_up(dza);
        if (lane >= 1 && lane < km) {
            const float dip = (qap1 - qa) / (dzap1 + dza);
            const float dim = (qa - qam1) / (dzam1 + dza);
            if (!(dip * dim <= 0.0f)) {
                qpi = qa + 0.5f * (dip + dim) * dza;
                qmi = 2.0f * qa - qpi;
                if (qpi < 0.0f || qmi < 0.0f) { qpi = qa; qmi = qa; }
            }
        }
    }
    const float zlo = zi, zhi = wsm_dn(zi);                  // the output cell of this lane is [zi(lane), zi(lane+1)]
    const float za_top = __shfl(za, km);
    // arrival heights below zlo among interfaces 1..km (nb) and below zhi among 0..km-1 (nt): za increases strictly, so each
    // count is the position of the first za >= z -- a 6-step binary search per lane instead of km+1 comparisons.  Both ranges hold
    // km <= 63 interfaces: six halvings settle fewer than 64 candidates, not 64 (a search over 0..km left lane 0 of a 63-level
    // column one candidate short whenever the lowest arrival height was below the ground and the next one above it).  The clamp of
    // the probed lane to 63 acts only where lo1 == hi1 == 64 (km = 63, every candidate below zlo): a settled search, whose probe
    // is read and discarded
    int lo1 = 1, hi1 = km + 1, lo2 = 0, hi2 = km;
    for (int step = 0; step < 6; ++step) {
        const int m1 = (lo1 + hi1) >> 1, m2 = (lo2 + hi2) >> 1;
        const float v1 = __shfl(za, m1 < 63 ? m1 : 63), v2 = __shfl(za, m2 < 63 ? m2 : 63);
        if (lo1 < hi1) { if (v1 < zlo) lo1 = m1 + 1; else hi1 = m1; }
        if (lo2 < hi2) { if (v2 < zhi) lo2 = m2 + 1; else hi2 = m2; }
    }
    const int nb = lo1 - 1, nt = lo2;
    const bool live = cell && !(zlo >= za_top);              // not yet `exit intp`
    const int kb = live ? nb + 1 : 1;                        // 1-based first kk with zi(k) <= za(kk+1); <= km when live
    const bool found = live && nt < km;                      // first kk with zi(k+1) <= za(kk) exists
    const int kt = found ? nt : 0;                           // that kk, minus 1
    const int ib = kb - 1, it = (kt >= 1 ? kt : 1) - 1;
    const float za_b = __shfl(za, ib), dza_b = __shfl(dza, ib), qpi_b = __shfl(qpi, ib), qmi_b = __shfl(qmi, ib), qa_b = __shfl(qa, ib);
    const float za_t = __shfl(za, it), dza_t = __shfl(dza, it), qpi_t = __shfl(qpi, it), qmi_t = __shfl(qmi, it);
    const float tl = (zlo - za_b) / dza_b;
    const float tl2 = tl * tl;
    const float qqd_b = 0.5f * (qpi_b - qmi_b);
    const float qql = qqd_b * tl2 + qmi_b * tl;
    float zsum = (1.f - tl) * dza_b, qsum = (qa_b - qql) * dza_b;
    const int cnt = (found && kt > kb) ? kt - kb - 1 : 0;    // m = kb+1 .. kt-1
    int cmax = cnt;
    for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(cmax, o); cmax = v > cmax ? v : cmax; }
    for (int s2 = 1; s2 <= cmax; ++s2) {
        const int m = kb + s2 - 1 <= 63 ? kb + s2 - 1 : 63;  // 0-based index of m = kb + s2
        const float dm = __shfl(dza, m), qm = __shfl(qa, m);
        if (s2 <= cnt) { zsum = zsum + dm; qsum = qsum + qm * dm; }
    }
    float qn = 0.0f;
    if (found && kt == kb) {
        const float th = (zhi - za_b) / dza_b;
        const float th2 = th * th;
        const float qqh = qqd_b * th2 + qmi_b * th;
        qn = (qqh - qql) / (th - tl);
    } else if (found && kt > kb) {
        const float th = (zhi - za_t) / dza_t;
        const float th2 = th * th;
        const float qqd = 0.5f * (qpi_t - qmi_t);
        const float dqh = qqd * th2 + qmi_t * th;
        zsum = zsum + th * dza_t;
        qsum = qsum + dqh * dza_t;
        qn = qsum / zsum;
    }
    for (int k = 0; k < km; ++k) {                           // rain out, k ascending (wave-uniform loop on broadcast values)
        const float zk = __shfl(za, k), zk1 = __shfl(za, k + 1), qk = __shfl(qa, k), dk = __shfl(dza, k);
        if (zk < 0.0f && zk1 < 0.0f) { precip = precip + qk * dk; continue; }
        else if (zk < 0.0f && zk1 >= 0.0f) { precip = precip + qk * (0.0f - zk); break; }
        break;
    }
    return qn;
}

// one column on one wave: lane = level for dz, den, denfac, tk, wwl (terminal velocity), rql[f] (den*q); zi = height of interface
// `lane` (0 at lane 0).  qn[f] = the fallen den*q of this lane's level, precip[f] = what left through the ground.
template <int NF, class Speed>
__device__ __forceinline__ void wsm_fall_wave(int km, int lane, float dz, float den, float denfac, float tk, float wwl, const float *rql, float zi,
                                              float dt, int iter, Speed speed, float *qn, float *precip)
{
    const bool cell = lane < km;
    bool some = false;
    for (int f = 0; f < NF; ++f) { precip[f] = 0.0f; qn[f] = rql[f]; some = some || rql[f] > 0.0f; }   // an empty column keeps den*q as it is (cycle i_loop)
    if (__ballot(cell && some) == 0ull) return;              // allold > 0: den*q >= 0, so the sum is positive iff one term is
    float ww = cell ? wwl : 0.0f, za, dza, qa[NF];
    for (int n = 1;; ++n) {
        wsm_wave_arrival(km, lane, ww, dz, zi, dt, za, dza);
        float q[NF];
        for (int f = 0; f < NF; ++f) qa[f] = cell ? rql[f] * dz / dza : 0.0f;   // qa(km+1) = 0
        if (n > iter) break;                                 // wave-uniform
        for (int f = 0; f < NF; ++f) q[f] = cell ? qa[f] / den : 0.f;
        const float wa = speed(q, den, denfac, tk);          // one refinement of the speed with the arrived mixing ratios
        ww = cell ? 0.5f * (wwl + wa) : 0.0f;
    }
    for (int f = 0; f < NF; ++f) qn[f] = wsm_wave_remap(km, lane, zi, za, dza, qa[f], precip[f]);
}
}  // namespace

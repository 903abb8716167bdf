// icar_amd/csrc/thompson_lane.inc -- Thompson column physics with ONE LEVEL PER THREAD.
// (included by mp_thompson.hip; reference: src/physics/mp_thompson.f90:1057-2844)
//
// The reference's column routine is ~95 % per-level work; what couples the levels is
//   * the graupel intercept's running minimum from the model top (:1456-1468, :2379-2391)  -> suffix-min
//   * fall speeds copied down from the nearest level that holds the species (:2544-2639)    -> carry-down
//   * ksed1 / nstep (:2548-2649)                                                             -> column max
//   * sedimentation fluxes from the level above, nstep sub-steps (:2660-2770)                -> neighbour read per sub-step
// With thread = level, every per-level array of the reference is a register.  The couplings go through a communicator policy
// (column_comm.h):
//   WaveComm  : one column per wave, level = lane; wave shuffles / ballot.  nz of 64 lanes are busy (used for 57 <= nz <= 64 and nz = 1: column_comm.h).
//   BlockComm : cpb whole columns per block, thread = level*cpb + column (column fastest: a wave spans few levels of neighbouring
//               columns => coalesced rows and little divergence); the couplings go through LDS.  240 of 256 threads busy at nz = 40.
// Round 5: every coupling reads DOWNWARD and what it carries can be posted before a barrier, so the block form needs five block
// barriers per column group (+ one per sedimentation sub-step; round 4: seventeen): any_min (:1363's any + the first chain's
// suffix-min), post_fall1 (second chain + carry-down of rain, ice, snow), post_fall2 (graupel), plan4, up6_of.
// All arithmetic is identical in both (min/max are order-independent; everything else is per thread).

// One level of one column per thread.  Inputs are this thread's level (idle threads carry a copy of a valid
// level and are masked out of every scan and store); outputs overwrite the inputs.
// graupel y-intercept before the running minimum (mp_thompson.f90:1456-1466)
__device__ __forceinline__ double th_graupel_N0_exp_k(const DK &K_, float rg, float xslw1)
{
    const float ygra1 = 4.31f + d_log10f(fmaxf(5.E-5f, rg));
    const float zans1 = 3.1f + (100.f / (300.f * xslw1 * ygra1 / (10.f / xslw1 + 1.f + 0.25f * ygra1) + 30.f + 10.f * ygra1));
    const double N0_exp = d_pow10f(zans1);
    return fmax((double)TH_gonv_min, fmin(N0_exp, (double)TH_gonv_max));
}

#define th_graupel_N0_exp(rg, xslw1) th_graupel_N0_exp_k(K_, (rg), (xslw1))

// What a level hands from its point physics (:1240-2650: working variables ... terminal fall speeds) to the sedimentation and
// the final update (:2660-2842): 25 REAL(4) values + the sedimentation plan's inputs.  Level-per-thread kernels keep it in
// registers (round 4 measured two lanes-along-i layouts that parked it in HBM / LDS instead: profiles/r04_thompson_layout.md).
struct ThHand {
    float vtrk, vtnrk, vtik, vtnik, vtsk, vtgk;                 /* fall speeds after the carry-down */
    float rr, nr, ri, ni, rs, rg;                               /* TAU+1 contents the sedimentation moves */
    float qrten, nrten, qiten, niten, qsten, qgten, qcten, qvten, tten;
    float rho, temp, ocp, lvap;
    int c4[4], ns4[4];                                          /* per species: a sedimenting particle here / its sub-step count */
};
#define TH_NHAND 25

// point physics of ONE level (:1240-2650).  Returns false when the whole column group has nothing to do (:1363).
template <class Comm>
__device__ __forceinline__ bool th_level_physics(const ThState *__restrict__ T, Comm &x, int nz, float dt, float dzq,
                               float &qv1d, float &qc1d, float &qi1d, float &qr1d, float &qs1d, float &qg1d, float &ni1d,
                               float &nr1d, float &t1d, float p1d, ThHand &h)
{
    const DK K_ = d_consts();

    const float *sa = T->sa, *sb = T->sb;
    const float R1 = TH_R1, R2 = TH_R2, eps = TH_eps, T_0 = TH_T_0, PI2 = TH_PI2;
    const float am_r = TH_am_r, am_i = TH_am_i, bm_i = TH_bm_i, bm_g = TH_bm_g, mu_i = TH_mu_i, mu_g = TH_mu_g;
    const float D0r = TH_D0r, D0c = TH_D0c, D0s = TH_D0s, D0g = TH_D0g, fv_r = TH_fv_r, lsub = TH_lsub, lvap0 = TH_lvap0;
    const float oRv = TH_oRv, olfus = TH_olfus, xm0i = TH_xm0i, C_cube = TH_C_cube, HGFR = TH_HGFR, rho_w = TH_rho_w;
    const float mu_r = T->mu_r, mu_c = T->mu_c, Nt_c = T->Nt_c, am_g = T->am_g, av_g = T->av_g, bv_g = T->bv_g;
    const float *ccg = T->ccg, *cie = T->cie, *cig = T->cig, *cre = T->cre, *crg = T->crg, *cge = T->cge, *cgg = T->cgg;
    const bool active = x.active;
    const float pres = p1d;

    float tten = 0, qvten = 0, qcten = 0, qiten = 0, qrten = 0, qsten = 0, qgten = 0, niten = 0, nrten = 0;
    float temp, qv, rc, ri, rr, rs, rg, ni, nr, rho, rhof, lvap = 0, ocp = 0, mvd_r, smob = 0, smoc = 0, xslw_arr = 0.01f, vts_boost = 1.5f;
    double ilamg, N0_g;
    int L_qc, L_qi, L_qr, L_qs, L_qg;
    float delta_tp, orho, lfus2;
    double N0_exp, N0_min, lam_exp, lamc, lamr, lamg, lami, ilami;
    GdLog Llamr; Llamr.hi = Llamr.lo = 0.;
    float xDc, Dc_b, Dc_g, xDi, xDs, xDg, zeta1, zeta, taud, tau, stoke_g;
    float vti, vtr, vts, vtg, Mrat, ils1, ils2, t1_vts, t2_vts, t3_vts, t4_vts, C_snow;
    float a_, b_, loga_, tf, tempc, tc0, xnc, xri, xni, xmi, oxmi, xrc, xrr, xnr;
    float xsat, rate_max, sump, ratio, clap, fcd, dfcd, otemp, rvs, rvs_p, rvs_pp, gamsc, alphsc, t1_evap, t1_subl;
    float r_frac, g_frac, Ef_rw, Ef_sw, Ef_gw = 0.f, Ef_rr, dtsave, odts, odt, xslw1;
    int n, idx_tc, idx_t, idx_s, idx_g1, idx_g, idx_r1, idx_r, idx_i1, idx_i, idx_c, idx;
    int no_micro = 1, lamr_same = 0, lami_same = 0;
    (void)vti; (void)vtr; (void)xnc; (void)sump; (void)odt;

    dtsave = dt; odt = 1.f / dt; odts = 1.f / dtsave;

    /* ---- :1240-1319 this level -> working variables ---- */
    {
        temp = t1d;
        qv = fmaxf(1.E-10f, qv1d);
        rho = 0.622f * pres / (TH_RR2 * temp * (qv + 0.622f));
        if (qc1d > R1) { no_micro = 0; rc = qc1d * rho; L_qc = 1; }
        else { qc1d = 0.0f; rc = R1; L_qc = 0; }
        if (qi1d > R1) {
            no_micro = 0;
            ri = qi1d * rho;
            ni = fmaxf(R2, ni1d * rho);
            L_qi = 1;
            lami = d_powf(am_i * cig[1] * T->oig1 * ni / ri, T->obmi);
            lami_same = 1;                                  /* the slope of (ni, ri) as they stand ... */
            ilami = 1. / lami;
            xDi = (float)((double)(bm_i + mu_i + 1.f) * ilami);
            if (xDi < 20.E-6f) {
                lami = cie[1] / 20.E-6f;
                ni = (float)fmin(250.e3, (double)(cig[0] * T->oig2 * ri / am_i) * (lami * lami * lami));
                lami_same = 0;                              /* ... unless the size limits moved ni */
            } else if (xDi > 300.E-6f) {
                lami = cie[1] / 300.E-6f;
                ni = (float)((double)(cig[0] * T->oig2 * ri / am_i) * (lami * lami * lami));
                lami_same = 0;
            }
        } else { qi1d = 0.0f; ni1d = 0.0f; ri = R1; ni = R2; L_qi = 0; }

        mvd_r = 0.0f;
        if (qr1d > R1) {
            no_micro = 0;
            rr = qr1d * rho;
            nr = fmaxf(R2, nr1d * rho);
            L_qr = 1;
            lamr = d_powf(am_r * crg[2] * T->org2 * nr / rr, T->obmr);
            lamr_same = 1;                                  /* the slope of (nr, rr) as they stand ... */
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r > 2.5E-3f) {
                mvd_r = 2.5E-3f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                nr = (float)((double)(crg[1] * T->org3 * rr) * (lamr * lamr * lamr) / (double)am_r);
                lamr_same = 0;                              /* ... unless the limits moved nr */
            } else if (mvd_r < D0r * 0.75f) {
                mvd_r = D0r * 0.75f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                nr = (float)((double)(crg[1] * T->org3 * rr) * (lamr * lamr * lamr) / (double)am_r);
                lamr_same = 0;
            }
        } else { qr1d = 0.0f; nr1d = 0.0f; rr = R1; nr = R2; L_qr = 0; }
        if (qs1d > R1) { no_micro = 0; rs = qs1d * rho; L_qs = 1; }
        else { qs1d = 0.0f; rs = R1; L_qs = 0; }
        if (qg1d > R1) { no_micro = 0; rg = qg1d * rho; L_qg = 1; }
        else { qg1d = 0.0f; rg = R1; L_qg = 0; }
        }
    /* no_micro needs the ice saturation of every level (:1345) */
    {
        const float tc_ = temp - 273.15f;
        const float qvs_ = rslf(pres, temp);
        const float qvsi_ = (tc_ <= 0.0f) ? rsif(pres, temp) : qvs_;
        float ssati_ = qv / qvsi_ - 1.f;
        if (fabsf(ssati_) < eps) ssati_ = 0.0f;
        if (ssati_ > 0.0f) no_micro = 0;
    }
    /* graupel y-intercept: N0_min is a running minimum from the model top down (:1456-1468 / :2379-2391)
     * = suffix-min over the levels of this column.  GRAUPEL_N0: the level's own value; GRAUPEL_SLOPE: slope / intercept from the
     * minimum, only read where graupel is present (rg > r_g(1), L_qg, rg > R1) */
#define GRAUPEL_N0(XSLW)                                                                                  \
    {                                                                                                \
        xslw1 = (XSLW);                                                                              \
        if (rg <= 5.E-5f && xslw1 == 0.01f) N0_exp = T->N0_exp_default;   /* same function, same arguments */ \
        else N0_exp = th_graupel_N0_exp(rg, xslw1);                                                  \
    }
#define GRAUPEL_SLOPE(VMIN)                                                                          \
    {                                                                                                \
        N0_min = fmin((VMIN), (double)TH_gonv_max);                                                  \
        N0_exp = N0_min;                                                                             \
        if (L_qg || rg > R1) {                                                                       \
            lam_exp = d_pow(N0_exp * am_g * cgg[0] / rg, (double)T->oge1);                           \
            lamg = lam_exp * T->pw_cgg_obmg;                 /* (cgg(3)*ogg2*ogg1)**obmg */                            \
            ilamg = 1. / lamg;                                                                       \
            N0_g = N0_exp / (cgg[1] * lam_exp) * d_pow(lamg, (double)cge[1]);                        \
        } else { lamg = 0.; ilamg = 0.; N0_g = 0.; }                                                 \
    }
    /* :1363 (nothing to do in the whole column group: uniform over the wave / block) and the first chain's minimum share one exchange */
    {
        GRAUPEL_N0((temp < 270.65f && L_qr && mvd_r > 100.E-6f) ? 4.01f + d_log10f(mvd_r) : 0.01f)
        double vmin_;
        if (!x.any_min(active && !no_micro, active ? N0_exp : (double)TH_gonv_max, vmin_)) return false;
        GRAUPEL_SLOPE(vmin_)
    }

    /* ---- per-level phase A: saturation, snow moments, rain slopes, warm rain, frozen processes,
     *      conservation, tendencies (:1328-2236) ---- */
    {
        double prr_wau = 0, prr_rcw = 0, prr_rcs = 0, prr_rcg = 0, prr_sml = 0, prr_gml = 0, prr_rci = 0, pnr_wau = 0, pnr_rcs = 0, pnr_rcg = 0, pnr_rci = 0, pnr_sml = 0, pnr_gml = 0, pnr_rcr = 0, pnr_rfz = 0, pri_inu = 0, pni_inu = 0, pri_ihm = 0, pni_ihm = 0, pri_wfz = 0, pni_wfz = 0, pri_rfz = 0, pni_rfz = 0, pri_ide = 0, pni_ide = 0, pri_rci = 0, pni_rci = 0, pni_sci = 0, pni_iau = 0, prs_iau = 0, prs_sci = 0, prs_rcs = 0, prs_scw = 0, prs_sde = 0, prs_ihm = 0, prs_ide = 0, prg_scw = 0, prg_rfz = 0, prg_gde = 0, prg_gcw = 0, prg_rci = 0, prg_rcs = 0, prg_rcg = 0, prg_ihm = 0;
        float rhof, rhof2, qvs, qvsi, delQvs, satw, sati, ssatw, ssati, diffu, visco, vsc2, tcond, lvap, ocp, mvd_c;
        float smob = 0.f, smo2 = 0.f, smo1 = 0.f, smo0 = 0.f, smoc = 0.f, smoe = 0.f, smof = 0.f;
        double ilamr, N0_r;
        (void)satw; (void)sati; (void)smo2;
        tempc = temp - 273.15f;
        rhof = sqrtf(TH_rho_not / rho);
        rhof2 = sqrtf(rhof);
        qvs = rslf(pres, temp);
        delQvs = fmaxf(0.0f, rslf(pres, 273.15f) - qv);
        if (tempc <= 0.0f) qvsi = rsif(pres, temp); else qvsi = qvs;
        satw = qv / qvs;
        sati = qv / qvsi;
        ssatw = satw - 1.f;
        ssati = sati - 1.f;
        if (fabsf(ssatw) < eps) ssatw = 0.0f;
        if (fabsf(ssati) < eps) ssati = 0.0f;
        diffu = 2.11E-5f * d_powf(temp / 273.15f, 1.94f) * (101325.f / pres);
        if (tempc >= 0.0f) visco = (1.718f + 0.0049f * tempc) * 1.0E-5f;
        else visco = (1.718f + 0.0049f * tempc - 1.2E-5f * tempc * tempc) * 1.0E-5f;
        ocp = 1.f / (TH_Cp2 * (1.f + 0.887f * qv));
        vsc2 = sqrtf(rho / visco);
        lvap = lvap0 + (2106.0f - 4218.0f) * tempc;
        tcond = (5.69f + 0.0168f * tempc) * 1.0E-5f * 418.936f;
            if (L_qs) {
        tc0 = fminf(-0.1f, temp - 273.15f);
        smob = rs * T->oams;
        if (TH_bm_s > (2.0f - 1.e-3f) && TH_bm_s < (2.0f + 1.e-3f)) smo2 = smob;
        else {
            loga_ = snow_poly_f(sa, tc0, TH_bm_s); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, TH_bm_s);
            smo2 = d_powf(smob / a_, 1.f / b_);
        }
        const PowBase Lsmo2 = d_powf_base(smo2);                  /* smo2 > 0: the five moments below are smo2**b_ */
        loga_ = sa[0] + sa[1] * tc0 + sa[4] * tc0 * tc0 + sa[8] * tc0 * tc0 * tc0;
        a_ = d_pow10f(loga_);
        b_ = sb[0] + sb[1] * tc0 + sb[4] * tc0 * tc0 + sb[8] * tc0 * tc0 * tc0;
        smo0 = a_ * d_powf_l(Lsmo2, b_);
        loga_ = sa[0] + sa[1] * tc0 + sa[2] + sa[3] * tc0 + sa[4] * tc0 * tc0 + sa[5] + sa[6] * tc0 * tc0 + sa[7] * tc0
              + sa[8] * tc0 * tc0 * tc0 + sa[9];
        a_ = d_pow10f(loga_);
        b_ = sb[0] + sb[1] * tc0 + sb[2] + sb[3] * tc0 + sb[4] * tc0 * tc0 + sb[5] + sb[6] * tc0 * tc0 + sb[7] * tc0
           + sb[8] * tc0 * tc0 * tc0 + sb[9];
        smo1 = a_ * d_powf_l(Lsmo2, b_);
        loga_ = snow_poly_f(sa, tc0, T->cse[0]); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, T->cse[0]);
        smoc = a_ * d_powf_l(Lsmo2, b_);
        loga_ = snow_poly_f(sa, tc0, T->cse[12]); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, T->cse[12]);
        smoe = a_ * d_powf_l(Lsmo2, b_);
        loga_ = snow_poly_f(sa, tc0, T->cse[15]); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, T->cse[15]);
        smof = a_ * d_powf_l(Lsmo2, b_);
            }
        /* rain slope, mean volume diameter, intercept: every later read is behind L_qr / rr >= r_r(1) */
        ilamr = 0.; N0_r = 0.;
        if (L_qr) {
            if (!lamr_same) lamr = d_powf(am_r * crg[2] * T->org2 * nr / rr, T->obmr);    /* else: same arguments as at :1285 */
            ilamr = 1. / lamr;
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            N0_r = (double)(nr * T->org2) * d_pow(lamr, (double)cre[1]);
        }
            if (L_qr && mvd_r > D0r) {
            Ef_rr = 2.0f - d_expf(2300.0f * (mvd_r - 1600.0E-6f));
            pnr_rcr = Ef_rr * 4.f * nr * rr;
        }
        mvd_c = D0c;
        if (L_qc) {
        xDc = fmaxf(D0c * 1.E6f, (d_powf(rc / (am_r * Nt_c), T->obmr)) * 1.E6f);
        lamc = d_powf(Nt_c * am_r * ccg[1] * T->ocg1 / rc, T->obmr);
        mvd_c = (float)((double)(3.0f + mu_c + 0.672f) / lamc);
        if (rc > 0.01e-3f) {
            Dc_g = (float)(((double)T->pw_ccg_obmr / lamc) * (double)1.E6f);   /* (ccg(3)*ocg2)**obmr */
            Dc_b = d_powf(xDc * xDc * xDc * Dc_g * Dc_g * Dc_g - xDc * xDc * xDc * xDc * xDc * xDc, 1.f / 6.f);
            zeta1 = 0.5f * ((6.25E-6f * xDc * Dc_b * Dc_b * Dc_b - 0.4f) + fabsf(6.25E-6f * xDc * Dc_b * Dc_b * Dc_b - 0.4f));
            zeta = 0.027f * rc * zeta1;
            taud = 0.5f * ((0.5f * Dc_b - 7.5f) + fabsf(0.5f * Dc_b - 7.5f)) + R1;
            tau = 3.72f / (rc * taud);
            prr_wau = zeta / tau;
            prr_wau = fmin((double)(rc * odts), prr_wau);
            pnr_wau = prr_wau / (double)(am_r * mu_c * D0r * D0r * D0r);
        }
        if (L_qr && mvd_r > D0r && mvd_c > D0c) {
            lamr = 1. / ilamr;
            idx = 1 + (int)(NBINS * d_log((double)mvd_r / T->Dr[0]) / T->log_Dr_span);
            idx = imin(idx, NBINS);
            int ic = (int)(mvd_c * 1.E6f);
            ic = imax(1, imin(ic, NBINS));          /* the reference does not bound this index */
            Ef_rw = (float)T->t_Efrw[(idx - 1) + NBINS * (ic - 1)];
            prr_rcw = (double)(rhof * T->t1_qr_qc * Ef_rw * rc) * N0_r * d_pow(lamr + (double)fv_r, -(double)cre[8]);
            prr_rcw = fmin((double)(rc * odts), prr_rcw);
        }
            }
        vts_boost = 1.5f;
        tempc = temp - 273.15f;
        idx_tc = imax(1, imin((int)lroundf(-tempc), 45));
        idx_t = (int)((tempc - 2.5f) / 5.f) - 1;
        idx_t = imax(1, -idx_t);
        idx_t = imin(idx_t, NTB_T);

        if (rc > T->r_c[0]) { idx_c = dec_index_f(T, rc, T->nic2); idx_c = imax(1, imin(idx_c, NTB_C)); } else idx_c = 1;
        if (ri > T->r_i[0]) { idx_i = dec_index_f(T, ri, T->nii2); idx_i = imax(1, imin(idx_i, NTB_I)); } else idx_i = 1;
        if (ni > T->Nt_i[0]) { idx_i1 = dec_index_f(T, ni, T->nii3); idx_i1 = imax(1, imin(idx_i1, NTB_I1)); } else idx_i1 = 1;
        if (rr > T->r_r[0]) {
            idx_r = dec_index_f(T, rr, T->nir2); idx_r = imax(1, imin(idx_r, NTB_R));
            lamr = 1. / ilamr;
            lam_exp = lamr * cube_f(crg[2] * T->org2 * T->org1);
            N0_exp = (double)(T->org1 * rr / am_r) * d_pow(lam_exp, (double)cre[0]);
            idx_r1 = dec_index_d(T, N0_exp, T->nir3); idx_r1 = imax(1, imin(idx_r1, NTB_R1));
        } else { idx_r = 1; idx_r1 = NTB_R1; }
        if (rs > T->r_s[0]) { idx_s = dec_index_f(T, rs, T->nis2); idx_s = imax(1, imin(idx_s, NTB_S)); } else idx_s = 1;
        if (rg > T->r_g[0]) {
            idx_g = dec_index_f(T, rg, T->nig2); idx_g = imax(1, imin(idx_g, NTB_G));
            lamg = 1. / ilamg;
            lam_exp = lamg * cube_f(cgg[2] * T->ogg2 * T->ogg1);
            N0_exp = (double)(T->ogg1 * rg / am_g) * d_pow(lam_exp, (double)cge[0]);
            idx_g1 = dec_index_d(T, N0_exp, T->nig3); idx_g1 = imax(1, imin(idx_g1, NTB_G1));
        } else { idx_g = 1; idx_g1 = NTB_G1; }

        /* deposition/sublimation prefactor :1679-1695 */
        otemp = 1.f / temp;
        rvs = rho * qvsi;
        rvs_p = rvs * otemp * (lsub * otemp * oRv - 1.f);
        rvs_pp = rvs * (otemp * (lsub * otemp * oRv - 1.f) * otemp * (lsub * otemp * oRv - 1.f)
                        + (-2.f * lsub * otemp * otemp * otemp * oRv) + otemp * otemp);
        gamsc = lsub * diffu / tcond * rvs_p;
        alphsc = 0.5f * (gamsc / (1.f + gamsc)) * (gamsc / (1.f + gamsc)) * rvs_pp / rvs_p * rvs / rvs_p;
        alphsc = fmaxf(1.E-9f, alphsc);
        xsat = ssati;
        if (fabsf(xsat) < 1.E-9f) xsat = 0.f;
        t1_subl = 4.f * PI2 * (1.0f - alphsc * xsat + 2.f * alphsc * alphsc * xsat * xsat
                               - 5.f * alphsc * alphsc * alphsc * xsat * xsat * xsat) / (1.f + gamsc);

        /* snow / graupel collecting cloud water :1698-1725 */
        if (L_qc && mvd_c > D0c) {
            xDs = 0.0f;
            if (L_qs) xDs = smoc / smob;
            if (xDs > D0s) {
                idx = 1 + (int)(NBINS * d_log((double)xDs / T->Ds[0]) / T->log_Ds_span);
                idx = imin(idx, NBINS);
                int ic = (int)(mvd_c * 1.E6f); ic = imax(1, imin(ic, NBINS));
                Ef_sw = (float)T->t_Efsw[(idx - 1) + NBINS * (ic - 1)];
                prs_scw = rhof * T->t1_qs_qc * Ef_sw * rc * smoe;
            }
            if (rg >= T->r_g[0] && mvd_c > D0c) {
                xDg = (float)((double)(bm_g + mu_g + 1.f) * ilamg);
                const GdLog Lig = d_plog(ilamg);                        /* rg >= r_g(1): ilamg > 0 */
                vtg = (float)((double)(rhof * av_g * cgg[5] * T->ogg3) * d_pow_l(Lig, (double)bv_g));
                stoke_g = mvd_c * mvd_c * vtg * rho_w / (9.f * visco * xDg);
                if (xDg > D0g) {
                    if (stoke_g >= 0.4f && stoke_g <= 10.f) Ef_gw = 0.55f * d_log10f(2.51f * stoke_g);
                    else if (stoke_g < 0.4f) Ef_gw = 0.0f;
                    else if (stoke_g > 10.f) Ef_gw = 0.77f;
                    prg_gcw = (double)(rhof * T->t1_qg_qc * Ef_gw * rc) * N0_g * d_pow_l(Lig, (double)cge[8]);
                }
            }
        }

        /* rain collecting snow / graupel :1730-1783 */
        if (rr >= T->r_r[0]) {
            if (rs >= T->r_s[0]) {
                if (temp < T_0) {
                    prr_rcs = -(T4S(tmr_racs2) + T4S(tcr_sacr2) + T4S(tmr_racs1) + T4S(tcr_sacr1));
                    prs_rcs = T4S(tmr_racs2) + T4S(tcr_sacr2) - T4S(tcs_racs1) - T4S(tms_sacr1);
                    prg_rcs = T4S(tmr_racs1) + T4S(tcr_sacr1) + T4S(tcs_racs1) + T4S(tms_sacr1);
                    prr_rcs = fmax((double)(-rr * odts), prr_rcs);
                    prs_rcs = fmax((double)(-rs * odts), prs_rcs);
                    prg_rcs = fmin((double)((rr + rs) * odts), prg_rcs);
                    pnr_rcs = T4S(tnr_racs1) + T4S(tnr_racs2) + T4S(tnr_sacr1) + T4S(tnr_sacr2);
                } else {
                    prs_rcs = -T4S(tcs_racs1) - T4S(tms_sacr1) + T4S(tmr_racs2) + T4S(tcr_sacr2);
                    prs_rcs = fmax((double)(-rs * odts), prs_rcs);
                    prr_rcs = -prs_rcs;
                    pnr_rcs = T4S(tnr_racs2) + T4S(tnr_sacr2);
                }
                pnr_rcs = fmin((double)(nr * odts), pnr_rcs);
            }
            if (rg >= T->r_g[0]) {
                if (temp < T_0) {
                    prg_rcg = T4G(tmr_racg) + T4G(tcr_gacr);
                    prg_rcg = fmin((double)(rr * odts), prg_rcg);
                    prr_rcg = -prg_rcg;
                    pnr_rcg = T4G(tnr_racg) + T4G(tnr_gacr);
                    pnr_rcg = fmin((double)(nr * odts), pnr_rcg);
                } else {
                    prr_rcg = T4G(tcg_racg);
                    prr_rcg = fmin((double)(rg * odts), prr_rcg);
                    prg_rcg = -prr_rcg;
                }
            }
        }

        if (temp < T_0) {      /* :1789-1949 sub-zero processes */
            vts_boost = 1.0f;
            rate_max = (qv - qvsi) * rho * odts * 0.999f;
            if (rr > T->r_r[0]) {
                prg_rfz = T3R(tpg_qrfz) * odts;
                pri_rfz = T3R(tpi_qrfz) * odts;
                pni_rfz = T3R(tni_qrfz) * odts;
                pnr_rfz = T3R(tnr_qrfz) * odts;
                pnr_rfz = fmin((double)(nr * odts), pnr_rfz);
            } else if (rr > R1 && temp < HGFR) {
                pri_rfz = rr * odts;
                pnr_rfz = nr * odts;
                pni_rfz = pnr_rfz;
            }
            if (rc > T->r_c[0]) {
                pri_wfz = T2C(tpi_qcfz) * odts;
                pri_wfz = fmin((double)(rc * odts), pri_wfz);
                pni_wfz = T2C(tni_qcfz) * odts;
                pni_wfz = fmin(fmin((double)(Nt_c * odts), pri_wfz / (double)(2.f * xm0i)), pni_wfz);
            } else if (rc > R1 && temp < HGFR) {
                pri_wfz = rc * odts;
                pni_wfz = fmin(fmin((double)(Nt_c * odts), pri_wfz / (double)(2.f * xm0i)), pni_wfz);
            }
            if ((ssati >= 0.25f) || (ssatw > eps && temp < 261.15f)) {
                xnc = fminf(250.E3f, T->TNO * d_expf(TH_ATO * (T_0 - temp)));
                xni = (float)((double)ni + (pni_rfz + pni_wfz) * (double)dtsave);
                pni_inu = 0.5f * (xnc - xni + fabsf(xnc - xni)) * odts;
                pri_inu = fmin((double)rate_max, (double)xm0i * pni_inu);
                pni_inu = pri_inu / (double)xm0i;
            }
            if (L_qi) {
                if (!lami_same) lami = d_powf(am_i * cig[1] * T->oig1 * ni / ri, T->obmi);    /* else: same arguments as at :1257 */
                ilami = 1. / lami;
                xDi = (float)fmax((double)T->D0i, (double)(bm_i + mu_i + 1.f) * ilami);
                xmi = am_i * (xDi * xDi * xDi);
                oxmi = 1.f / xmi;
                pri_ide = (double)(C_cube * t1_subl * diffu * ssati * rvs * T->oig1 * cig[4] * ni) * ilami;
                if (pri_ide < 0.0) {
                    pri_ide = fmax(fmax((double)(-ri * odts), pri_ide), (double)rate_max);
                    pni_ide = pri_ide * (double)oxmi;
                    pni_ide = fmax((double)(-ni * odts), pni_ide);
                } else {
                    pri_ide = fmin(pri_ide, (double)rate_max);
                    prs_ide = (1.0 - T2I(tpi_ide)) * pri_ide;
                    pri_ide = T2I(tpi_ide) * pri_ide;
                }
                if ((idx_i == NTB_I) || (xDi > 5.0f * D0s)) {
                    prs_iau = ri * .99f * odts;
                    pni_iau = ni * .95f * odts;
                } else if (xDi < 0.1f * D0s) {
                    prs_iau = 0.; pni_iau = 0.;
                } else {
                    prs_iau = T2I(tps_iaus) * odts;
                    prs_iau = fmin((double)(ri * .99f * odts), prs_iau);
                    pni_iau = T2I(tni_iaus) * odts;
                    pni_iau = fmin((double)(ni * .95f * odts), pni_iau);
                }
            }
            if (L_qs) {
                C_snow = T->C_sqrd + (tempc + 15.f) * (T->C_cubes - T->C_sqrd) / (-30.f + 15.f);
                C_snow = fmaxf(T->C_sqrd, fminf(C_snow, T->C_cubes));
                prs_sde = C_snow * t1_subl * diffu * ssati * rvs
                             * (T->t1_qs_sd * smo1 + T->t2_qs_sd * rhof2 * vsc2 * smof);
                if (prs_sde < 0.) prs_sde = fmax(fmax((double)(-rs * odts), prs_sde), (double)rate_max);
                else prs_sde = fmin(prs_sde, (double)rate_max);
            }
            if (L_qg && ssati < -eps) {
                const GdLog Lig = d_plog(ilamg);                        /* L_qg: ilamg > 0 */
                prg_gde = (double)(C_cube * t1_subl * diffu * ssati * rvs) * N0_g
                             * ((double)T->t1_qg_sd * d_pow_l(Lig, (double)cge[9])
                                + (double)(T->t2_qg_sd * vsc2 * rhof2) * d_pow_l(Lig, (double)cge[10]));
                if (prg_gde < 0.) prg_gde = fmax(fmax((double)(-rg * odts), prg_gde), (double)rate_max);
                else prg_gde = fmin(prg_gde, (double)rate_max);
            }
            if (L_qi) {
                /* lami, ilami, xDi, xmi, oxmi: the values of the deposition block above (same ni, ri) */
                if (rs >= T->r_s[0]) {
                    prs_sci = T->t1_qs_qi * rhof * T->Ef_si * ri * smoe;
                    pni_sci = prs_sci * (double)oxmi;
                }
                if (rr >= T->r_r[0] && mvd_r > 4.f * xDi) {
                    lamr = 1. / ilamr;
                    const GdLog Llf = d_plog(lamr + (double)fv_r); const double pw8 = d_pow_l(Llf, -(double)cre[8]);
                    pri_rci = (double)(rhof * T->t1_qr_qi * T->Ef_ri * ri) * N0_r * pw8;
                    pnr_rci = (double)(rhof * T->t1_qr_qi * T->Ef_ri * ni) * N0_r * pw8;
                    pni_rci = pri_rci * (double)oxmi;
                    prr_rci = (double)(rhof * T->t2_qr_qi * T->Ef_ri * ni) * N0_r * d_pow_l(Llf, -(double)cre[7]);
                    prr_rci = fmin((double)(rr * odts), prr_rci);
                    prg_rci = pri_rci + prr_rci;
                }
            }
            if (prg_gcw > (double)eps && tempc > -8.0f) {
                tf = 0.f;
                if (tempc >= -5.0f && tempc < -3.0f) tf = 0.5f * (-3.0f - tempc);
                else if (tempc > -8.0f && tempc < -5.0f) tf = 0.33333333f * (8.0f + tempc);
                pni_ihm = (double)(3.5E8f * tf) * prg_gcw;
                pri_ihm = (double)xm0i * pni_ihm;
                prs_ihm = prs_scw / (prs_scw + prg_gcw) * pri_ihm;
                prg_ihm = prg_gcw / (prs_scw + prg_gcw) * pri_ihm;
            }
            if (prs_scw > (double)5.0f * prs_sde && prs_sde > (double)eps) {
                r_frac = (float)fmin(30.0, prs_scw / prs_sde);
                g_frac = fminf(0.75f, 0.05f + (r_frac - 5.f) * .028f);
                vts_boost = fminf(1.5f, 1.1f + (r_frac - 5.f) * .016f);
                prg_scw = (double)g_frac * prs_scw;
                prs_scw = (double)(1.f - g_frac) * prs_scw;
            }
        } else {                  /* :1953-2005 melting */
            if (L_qs) {
                prr_sml = (tempc * tcond - lvap0 * diffu * delQvs)
                             * (T->t1_qs_me * smo1 + T->t2_qs_me * rhof2 * vsc2 * smof);
                prr_sml = prr_sml + (double)(4218.f * olfus * tempc) * (prr_rcs + prs_scw);
                prr_sml = fmin((double)(rs * odts), fmax(0., prr_sml));
                pnr_sml = (double)(smo0 / rs) * prr_sml * (double)d_pow10f(-0.75f * tempc);
                pnr_sml = fmin((double)(smo0 * odts), pnr_sml);
                if (tempc > 3.5f || rs < 0.005E-3f) pnr_sml = 0.0;
                if (ssati < 0.f) {
                    prs_sde = T->C_cubes * t1_subl * diffu * ssati * rvs
                                 * (T->t1_qs_sd * smo1 + T->t2_qs_sd * rhof2 * vsc2 * smof);
                    prs_sde = fmax((double)(-rs * odts), prs_sde);
                }
            }
            if (L_qg) {
                const GdLog Lig = d_plog(ilamg); const double pw9 = d_pow_l(Lig, (double)cge[9]), pw10 = d_pow_l(Lig, (double)cge[10]);
                prr_gml = (double)(tempc * tcond - lvap0 * diffu * delQvs) * N0_g
                             * ((double)T->t1_qg_me * pw9
                                + (double)(T->t2_qg_me * rhof2 * vsc2) * pw10);
                prr_gml = fmin((double)(rg * odts), fmax(0., prr_gml));
                pnr_gml = N0_g * (double)cgg[1] * d_pow_lx(Lig, ilamg, (double)cge[1]) / (double)rg
                             * prr_gml * (double)d_pow10f(-1.5f * tempc);
                if (tempc > 7.5f || rg < 0.005E-3f) pnr_gml = 0.0;
                if (ssati < 0.f) {
                    prg_gde = (double)(C_cube * t1_subl * diffu * ssati * rvs) * N0_g
                                 * ((double)T->t1_qg_sd * pw9
                                    + (double)(T->t2_qg_sd * vsc2 * rhof2) * pw10);
                    prg_gde = fmax((double)(-rg * odts), prg_gde);
                }
            }
            if (dt > 120.f) {
                prr_rcw = prr_rcw + prs_scw + prg_gcw;
                prs_scw = 0.; prg_gcw = 0.;
            }
        }
            sump = (float)(pri_inu + pri_ide + prs_ide + prs_sde + prg_gde);
        rate_max = (qv - qvsi) * odts * 0.999f;
        if ((sump > eps && sump > rate_max) || (sump < -eps && sump < rate_max)) {
            ratio = rate_max / sump;
            pri_inu *= ratio; pri_ide *= ratio; pni_ide *= ratio; prs_ide *= ratio; prs_sde *= ratio; prg_gde *= ratio;
        }
        sump = (float)(-prr_wau - pri_wfz - prr_rcw - prs_scw - prg_scw - prg_gcw);
        rate_max = -rc * odts;
        if (sump < rate_max && L_qc) {
            ratio = rate_max / sump;
            prr_wau *= ratio; pri_wfz *= ratio; prr_rcw *= ratio; prs_scw *= ratio; prg_scw *= ratio; prg_gcw *= ratio;
        }
        sump = (float)(pri_ide - prs_iau - prs_sci - pri_rci);
        rate_max = -ri * odts;
        if (sump < rate_max && L_qi) {
            ratio = rate_max / sump;
            pri_ide *= ratio; prs_iau *= ratio; prs_sci *= ratio; pri_rci *= ratio;
        }
        sump = (float)(-prg_rfz - pri_rfz - prr_rci + prr_rcs + prr_rcg);
        rate_max = -rr * odts;
        if (sump < rate_max && L_qr) {
            ratio = rate_max / sump;
            prg_rfz *= ratio; pri_rfz *= ratio; prr_rci *= ratio; prr_rcs *= ratio; prr_rcg *= ratio;
        }
        sump = (float)(prs_sde - prs_ihm - prr_sml + prs_rcs);
        rate_max = -rs * odts;
        if (sump < rate_max && L_qs) {
            ratio = rate_max / sump;
            prs_sde *= ratio; prs_ihm *= ratio; prr_sml *= ratio; prs_rcs *= ratio;
        }
        sump = (float)(prg_gde - prg_ihm - prr_gml + prg_rcg);
        rate_max = -rg * odts;
        if (sump < rate_max && L_qg) {
            ratio = rate_max / sump;
            prg_gde *= ratio; prg_ihm *= ratio; prr_gml *= ratio; prg_rcg *= ratio;
        }
        pri_ihm = prs_ihm + prg_ihm;
        ratio = (float)fmin(fabs(prr_rcg), fabs(prg_rcg));
        prr_rcg = ratio * copysignf(1.0f, (float)prr_rcg);
        prg_rcg = -prr_rcg;
        if (temp > T_0) {
            ratio = (float)fmin(fabs(prr_rcs), fabs(prs_rcs));
            prr_rcs = ratio * copysignf(1.0f, (float)prr_rcs);
            prs_rcs = -prr_rcs;
        }
            orho = 1.f / rho;
        lfus2 = lsub - lvap;
        qvten = (float)(qvten + (-pri_inu - pri_ide - prs_ide - prs_sde - prg_gde) * orho);
        qcten = (float)(qcten + (-prr_wau - pri_wfz - prr_rcw - prs_scw - prg_scw - prg_gcw) * orho);
        qiten = (float)(qiten + (pri_inu + pri_ihm + pri_wfz + pri_rfz + pri_ide
                                       - prs_iau - prs_sci - pri_rci) * orho);
        niten = (float)(niten + (pni_inu + pni_ihm + pni_wfz + pni_rfz + pni_ide
                                       - pni_iau - pni_sci - pni_rci) * orho);
        xri = fmaxf(R1, (qi1d + qiten * dtsave) * rho);
        xni = fmaxf(R2, (ni1d + niten * dtsave) * rho);
        if (xri > R1) {
            lami = d_powf(am_i * cig[1] * T->oig1 * xni / xri, T->obmi);
            ilami = 1. / lami;
            xDi = (float)((double)(bm_i + mu_i + 1.f) * ilami);
            if (xDi < 20.E-6f) {
                lami = cie[1] / 20.E-6f;
                xni = (float)fmin(250.e3, (double)(cig[0] * T->oig2 * xri / am_i) * (lami * lami * lami));
                niten = (xni - ni1d * rho) * odts * orho;
            } else if (xDi > 300.E-6f) {
                lami = cie[1] / 300.E-6f;
                xni = (float)((double)(cig[0] * T->oig2 * xri / am_i) * (lami * lami * lami));
                niten = (xni - ni1d * rho) * odts * orho;
            }
        } else niten = -ni1d * odts;
        xni = fmaxf(0.f, (ni1d + niten * dtsave) * rho);
        if (xni > 250.E3f) niten = (250.E3f - ni1d * rho) * odts * orho;

        qrten = (float)(qrten + (prr_wau + prr_rcw + prr_sml + prr_gml + prr_rcs + prr_rcg
                                       - prg_rfz - pri_rfz - prr_rci) * orho);
        nrten = (float)(nrten + (pnr_wau + pnr_sml + pnr_gml
                                       - (pnr_rfz + pnr_rcr + pnr_rcg + pnr_rcs + pnr_rci)) * orho);
        xrr = fmaxf(R1, (qr1d + qrten * dtsave) * rho);
        xnr = fmaxf(R2, (nr1d + nrten * dtsave) * rho);
        if (xrr > R1) {
            lamr = d_powf(am_r * crg[2] * T->org2 * xnr / xrr, T->obmr);
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r > 2.5E-3f) {
                mvd_r = 2.5E-3f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                xnr = (float)((double)(crg[1] * T->org3 * xrr) * (lamr * lamr * lamr) / (double)am_r);
                nrten = (xnr - nr1d * rho) * odts * orho;
            } else if (mvd_r < D0r * 0.75f) {
                mvd_r = D0r * 0.75f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                xnr = (float)((double)(crg[1] * T->org3 * xrr) * (lamr * lamr * lamr) / (double)am_r);
                nrten = (xnr - nr1d * rho) * odts * orho;
            }
        } else { qrten = -qr1d * odts; nrten = -nr1d * odts; }

        qsten = (float)(qsten + (prs_iau + prs_sde + prs_sci + prs_scw + prs_rcs + prs_ide
                                       - prs_ihm - prr_sml) * orho);
        qgten = (float)(qgten + (prg_scw + prg_rfz + prg_gde + prg_rcg + prg_gcw + prg_rci
                                       + prg_rcs - prg_ihm - prr_gml) * orho);
        if (temp < T_0) {
            tten = (float)(tten + ((double)(lsub * ocp) * (pri_inu + pri_ide + prs_ide + prs_sde + prg_gde)
                              + (double)(lfus2 * ocp) * (pri_wfz + pri_rfz + prg_rfz + prs_scw + prg_scw + prg_gcw
                                                             + prg_rcs + prs_rcs + prr_rci + prg_rcg)) * orho * 1);
        } else {
            tten = (float)(tten + ((double)(TH_lfus * ocp) * (-prr_sml - prr_gml - prr_rcg - prr_rcs)
                              + (double)(lsub * ocp) * (prs_sde + prg_gde)) * orho * 1);
        }
        }

    /* ---- per-level phase B: TAU+1 state, condensation, rain evaporation (:2241-2505) ---- */
    {
        float rhof, rhof2, qvs, ssatw, diffu, visco, vsc2, tcond, lvt2, smo2 = 0.f, smod = 0.f;
        double ilamr, N0_r, prw_vcd = 0, prv_rev = 0, pnr_rev = 0;
        Llamr.hi = Llamr.lo = 0.;
        (void)rhof2; (void)smod; (void)prv_rev; (void)rhof;
        temp = t1d + dt * tten;
        otemp = 1.f / temp;
        tempc = temp - 273.15f;
        qv = fmaxf(1.E-10f, qv1d + dt * qvten);
        rho = 0.622f * pres / (TH_RR2 * temp * (qv + 0.622f));
        rhof = sqrtf(TH_rho_not / rho);
        rhof2 = sqrtf(rhof);
        qvs = rslf(pres, temp);
        ssatw = qv / qvs - 1.f;
        if (fabsf(ssatw) < eps) ssatw = 0.0f;
        diffu = 2.11E-5f * d_powf(temp / 273.15f, 1.94f) * (101325.f / pres);
        if (tempc >= 0.0f) visco = (1.718f + 0.0049f * tempc) * 1.0E-5f;
        else visco = (1.718f + 0.0049f * tempc - 1.2E-5f * tempc * tempc) * 1.0E-5f;
        vsc2 = sqrtf(rho / visco);
        lvap = lvap0 + (2106.0f - 4218.0f) * tempc;
        tcond = (5.69f + 0.0168f * tempc) * 1.0E-5f * 418.936f;
        ocp = 1.f / (TH_Cp2 * (1.f + 0.887f * qv));
        lvt2 = lvap * lvap * ocp * oRv * otemp * otemp;

        if ((qc1d + qcten * dt) > R1) { rc = (qc1d + qcten * dt) * rho; L_qc = 1; }
        else { rc = R1; L_qc = 0; }
        if ((qi1d + qiten * dt) > R1) {
            ri = (qi1d + qiten * dt) * rho;
            ni = fmaxf(R2, (ni1d + niten * dt) * rho);
            L_qi = 1;
        } else { ri = R1; ni = R2; L_qi = 0; }
        if ((qr1d + qrten * dt) > R1) {
            rr = (qr1d + qrten * dt) * rho;
            nr = fmaxf(R2, (nr1d + nrten * dt) * rho);
            L_qr = 1;
            lamr = d_powf(am_r * crg[2] * T->org2 * nr / rr, T->obmr);
            lamr_same = 1;
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r > 2.5E-3f) {
                mvd_r = 2.5E-3f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                nr = (float)((double)(crg[1] * T->org3 * rr) * (lamr * lamr * lamr) / (double)am_r);
                lamr_same = 0;
            } else if (mvd_r < D0r * 0.75f) {
                mvd_r = D0r * 0.75f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r;
                nr = (float)((double)(crg[1] * T->org3 * rr) * (lamr * lamr * lamr) / (double)am_r);
                lamr_same = 0;
            }
        } else { rr = R1; nr = R2; L_qr = 0; lamr_same = 0; }
        if ((qs1d + qsten * dt) > R1) { rs = (qs1d + qsten * dt) * rho; L_qs = 1; }
        else { rs = R1; L_qs = 0; }
        if ((qg1d + qgten * dt) > R1) { rg = (qg1d + qgten * dt) * rho; L_qg = 1; }
        else { rg = R1; L_qg = 0; }
            if (L_qs) {
        tc0 = fminf(-0.1f, temp - 273.15f);
        smob = rs * T->oams;
        if (TH_bm_s > (2.0f - 1.e-3f) && TH_bm_s < (2.0f + 1.e-3f)) smo2 = smob;
        else {
            loga_ = snow_poly_f(sa, tc0, TH_bm_s); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, TH_bm_s);
            smo2 = d_powf(smob / a_, 1.f / b_);
        }
        const PowBase Lsmo2 = d_powf_base(smo2);
        loga_ = snow_poly_f(sa, tc0, T->cse[0]); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, T->cse[0]);
        smoc = a_ * d_powf_l(Lsmo2, b_);
        loga_ = snow_poly_f(sa, tc0, T->cse[13]); a_ = d_pow10f(loga_); b_ = snow_poly_f(sb, tc0, T->cse[13]);
        smod = a_ * d_powf_l(Lsmo2, b_);
            }
        /* input of the second graupel chain (:2381-2385) must see the TAU+1 state of THIS point in the sequence */
        xslw_arr = (temp < 270.65f && L_qr && mvd_r > 100.E-6f) ? 4.01f + d_log10f(mvd_r) : 0.01f;
        ilamr = 0.; N0_r = 0.;
        if (L_qr) {
            if (!lamr_same) lamr = d_powf(am_r * crg[2] * T->org2 * nr / rr, T->obmr);
            Llamr = d_plog(lamr);
            ilamr = 1. / lamr;
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            N0_r = (double)(nr * T->org2) * d_pow_lx(Llamr, lamr, (double)cre[1]);
            lamr_same = 1;                                  /* lamr, Llamr belong to (nr, rr) until the evaporation below moves them */
        }
            if ((ssatw > eps) || (ssatw < -eps && L_qc)) {
            clap = (qv - qvs) / (1.f + lvt2 * qvs);
            for (n = 1; n <= 3; ++n) {
                const float ex_ = d_expf(lvt2 * clap);
                fcd = qvs * ex_ - qv + clap;
                dfcd = qvs * lvt2 * ex_ + 1.f;
                clap = clap - fcd / dfcd;
            }
            xrc = rc + clap;
            if (xrc > 0.0f) prw_vcd = clap * odt;
            else prw_vcd = -rc / rho * odts;
            qcten = (float)(qcten + prw_vcd);
            qvten = (float)(qvten - prw_vcd);
            tten = (float)(tten + (double)(lvap * ocp) * prw_vcd * 1);
            rc = fmaxf(R1, (qc1d + dt * qcten) * rho);
            qv = fmaxf(1.E-10f, qv1d + dt * qvten);
            temp = t1d + dt * tten;
            rho = 0.622f * pres / (TH_RR2 * temp * (qv + 0.622f));
            qvs = rslf(pres, temp);
            ssatw = qv / qvs - 1.f;
        }
            if ((ssatw < -eps) && L_qr && (!(prw_vcd > 0.))) {
            tempc = temp - 273.15f;
            otemp = 1.f / temp;
            rhof = sqrtf(TH_rho_not / rho);
            rhof2 = sqrtf(rhof);
            diffu = 2.11E-5f * d_powf(temp / 273.15f, 1.94f) * (101325.f / pres);
            if (tempc >= 0.0f) visco = (1.718f + 0.0049f * tempc) * 1.0E-5f;
            else visco = (1.718f + 0.0049f * tempc - 1.2E-5f * tempc * tempc) * 1.0E-5f;
            vsc2 = sqrtf(rho / visco);
            lvap = lvap0 + (2106.0f - 4218.0f) * tempc;
            tcond = (5.69f + 0.0168f * tempc) * 1.0E-5f * 418.936f;
            ocp = 1.f / (TH_Cp2 * (1.f + 0.887f * qv));
            rvs = rho * qvs;
            rvs_p = rvs * otemp * (lvap * otemp * oRv - 1.f);
            rvs_pp = rvs * (otemp * (lvap * otemp * oRv - 1.f) * otemp * (lvap * otemp * oRv - 1.f)
                            + (-2.f * lvap * otemp * otemp * otemp * oRv) + otemp * otemp);
            gamsc = lvap * diffu / tcond * rvs_p;
            alphsc = 0.5f * (gamsc / (1.f + gamsc)) * (gamsc / (1.f + gamsc)) * rvs_pp / rvs_p * rvs / rvs_p;
            alphsc = fmaxf(1.E-9f, alphsc);
            xsat = fminf(-1.E-9f, ssatw);
            t1_evap = 2.f * PI2 * (1.0f - alphsc * xsat + 2.f * alphsc * alphsc * xsat * xsat
                                   - 5.f * alphsc * alphsc * alphsc * xsat * xsat * xsat) / (1.f + gamsc);
            lamr = 1. / ilamr;
            if (qv / qvs < 0.95f && rr / rho <= 1.E-8f) {
                prv_rev = rr / rho * odts;
            } else {
                prv_rev = (double)(t1_evap * diffu * (-ssatw)) * N0_r * (double)rvs
                             * ((double)T->t1_qr_ev * d_pow(ilamr, (double)cre[9])
                                + (double)(T->t2_qr_ev * vsc2 * rhof2) * d_pow(lamr + (double)(0.5f * fv_r), -(double)cre[10]));
                rate_max = fminf((rr / rho * odts), (qvs - qv) * odts);
                prv_rev = fmin((double)rate_max, prv_rev / (double)rho);
            }
            pnr_rev = fmin((double)(nr * 0.99f / rho * odts), prv_rev * (double)nr / (double)rr);
            qrten = (float)(qrten - prv_rev);
            qvten = (float)(qvten + prv_rev);
            nrten = (float)(nrten - pnr_rev);
            tten = (float)(tten - (double)(lvap * ocp) * prv_rev * 1);
            rr = fmaxf(R1, (qr1d + dt * qrten) * rho);
            qv = fmaxf(1.E-10f, qv1d + dt * qvten);
            nr = fmaxf(R2, (nr1d + dt * nrten) * rho);
            lamr_same = 0;
            temp = t1d + dt * tten;
            rho = 0.622f * pres / (TH_RR2 * temp * (qv + 0.622f));
        }
        }
    /* ---- :2379-2391 second graupel chain and :2515-2650 terminal fall speeds.  vtXk(k) = vtXk(k+1) where the species is absent
     * (:2544, :2576, :2613, :2639) is "the value of the nearest level above that holds the species".  Exchange 1 carries the
     * chain's minimum and everything that does not depend on it: rain, cloud ice, and snow BEFORE its max with the rain speed
     * of its own level (:2606 -- the reader applies it: it sees that level's rain speed and T > T_0 flag too); exchange 2 the
     * graupel speed, which needs the slope the minimum gives; then ksed1 / nstep. ---- */
    float vtrk, vtnrk, vtik, vtnik, vtsk, vtgk;
    int c4[4], ns4[4] = {0, 0, 0, 0};
    {
        GRAUPEL_N0(xslw_arr)
        rhof = sqrtf(TH_rho_not / rho);
        const int has_r = active && (rr > R1), has_i = active && (ri > R1), has_s = active && (rs > R1), has_g = active && (rg > R1);
        const int warm = temp > T_0;
        float a_r = 0.f, b_r = 0.f, a_i = 0.f, b_i = 0.f, a_s = 0.f, a_g = 0.f;
        if (has_r) {
            if (!lamr_same) { lamr = d_powf(am_r * crg[2] * T->org2 * nr / rr, T->obmr); Llamr = d_plog(lamr); }
            const GdLog Llf = d_plog(lamr + (double)fv_r);
            a_r = (float)((double)(rhof * TH_av_r * crg[5] * T->org3) * d_pow_l(Llamr, (double)cre[2]) * d_pow_l(Llf, -(double)cre[5]));
            b_r = (float)((double)(rhof * TH_av_r * crg[6] / crg[11]) * d_pow_l(Llamr, (double)cre[11]) * d_pow_l(Llf, -(double)cre[6]));
        }
        if (has_i) {
            lami = d_powf(am_i * cig[1] * T->oig1 * ni / ri, T->obmi);
            ilami = 1. / lami;
            a_i = (float)((double)(rhof * T->av_i * cig[2] * T->oig2) * ilami);
            b_i = (float)((double)(rhof * T->av_i * cig[5] / cig[6]) * ilami);
        }
        if (has_s) {
            xDs = smoc / smob;
            Mrat = 1.f / xDs;
            ils1 = 1.f / (Mrat * TH_Lam0 + T->fv_s);
            ils2 = 1.f / (Mrat * TH_Lam1 + T->fv_s);
            const float Mrat_mu = d_powf(Mrat, TH_mu_s);
            t1_vts = TH_Kap0 * T->csg[3] * d_powf(ils1, T->cse[3]);
            t2_vts = TH_Kap1 * Mrat_mu * T->csg[9] * d_powf(ils2, T->cse[9]);
            ils1 = 1.f / (Mrat * TH_Lam0);
            ils2 = 1.f / (Mrat * TH_Lam1);
            t3_vts = TH_Kap0 * T->csg[0] * d_powf(ils1, T->cse[0]);
            t4_vts = TH_Kap1 * Mrat_mu * T->csg[6] * d_powf(ils2, T->cse[6]);
            vts = rhof * T->av_s * (t1_vts + t2_vts) / (t3_vts + t4_vts);
            a_s = vts * vts_boost;
        }
        {
            const float pv_[5] = {a_r, b_r, a_i, b_i, a_s};
            const int hs_[5] = {has_r, has_i, has_s, has_g, warm};
            x.post_fall1(active ? N0_exp : (double)TH_gonv_max, pv_, hs_);
        }
        const int k_ = x.k;
        /* rain and cloud ice */
        {
            const int kr = x.above(0, k_), ki = x.above(1, k_), krc = kr < 0 ? k_ : kr, kic = ki < 0 ? k_ : ki;
            const float pr0 = x.peek(0, krc), pr1 = x.peek(1, krc), pi0 = x.peek(2, kic), pi1 = x.peek(3, kic);
            vtrk = has_r ? a_r : (kr >= 0 ? pr0 : 0.f); vtnrk = has_r ? b_r : (kr >= 0 ? pr1 : 0.f);
            vtik = has_i ? a_i : (ki >= 0 ? pi0 : 0.f); vtnik = has_i ? b_i : (ki >= 0 ? pi1 : 0.f);
        }
        /* snow: a level that holds snow takes max(vts * vts_boost, vtrk) where T > T_0 (:2606); a level without snow copies that
         * of the nearest snow level above, whose own rain speed is its a_r or the one it copied from above */
        {
            const int ks = x.above(2, k_), ksc = ks < 0 ? k_ : ks;
            const float ps = x.peek(4, ksc);
            const int krs = x.bit(0, ksc) ? ksc : x.above(0, ksc), krsc = krs < 0 ? k_ : krs;
            const float prs = x.peek(0, krsc);
            const float vtr_ks = krs >= 0 ? prs : 0.f;
            const float as_ks = x.bit(4, ksc) ? fmaxf(ps, vtr_ks) : ps;
            vtsk = has_s ? (warm ? fmaxf(a_s, vtrk) : a_s) : (ks >= 0 ? as_ks : 0.f);
        }
        /* graupel: the chain's minimum -> slope -> speed */
        GRAUPEL_SLOPE(x.min_fall1())
        (void)N0_g;
        if (has_g) {
            vtg = (float)((double)(rhof * av_g * cgg[5] * T->ogg3) * d_pow(ilamg, (double)bv_g));
            a_g = warm ? fmaxf(vtg, vtrk) : vtg;
        }
        x.post_fall2(a_g);
        {
            const int kg = x.above(3, k_), kgc = kg < 0 ? k_ : kg;
            const float pg = x.peek(5, kgc);
            vtgk = has_g ? a_g : (kg >= 0 ? pg : 0.f);
        }
        c4[0] = active && (fmaxf(vtrk, vtnrk) > 1.E-3f);
        if (c4[0]) { delta_tp = dzq / fmaxf(vtrk, vtnrk); ns4[0] = (int)(dt / delta_tp + 1.f); }
        c4[1] = active && (vtik > 1.E-3f);
        if (c4[1]) { delta_tp = dzq / vtik; ns4[1] = (int)(dt / delta_tp + 1.f); }
        c4[2] = active && (vtsk > 1.E-3f);
        if (c4[2]) { delta_tp = dzq / vtsk; ns4[2] = (int)(dt / delta_tp + 1.f); }
        c4[3] = active && (vtgk > 1.E-3f);
        if (c4[3]) { delta_tp = dzq / vtgk; ns4[3] = (int)(dt / delta_tp + 1.f); }
    }
    h.vtrk = vtrk; h.vtnrk = vtnrk; h.vtik = vtik; h.vtnik = vtnik; h.vtsk = vtsk; h.vtgk = vtgk;
    h.rr = rr; h.nr = nr; h.ri = ri; h.ni = ni; h.rs = rs; h.rg = rg;
    h.qrten = qrten; h.nrten = nrten; h.qiten = qiten; h.niten = niten; h.qsten = qsten; h.qgten = qgten;
    h.qcten = qcten; h.qvten = qvten; h.tten = tten;
    h.rho = rho; h.temp = temp; h.ocp = ocp; h.lvap = lvap;
    for (int s = 0; s < 4; ++s) { h.c4[s] = c4[s]; h.ns4[s] = ns4[s]; }
    return true;
}

// :2660-2770 sedimentation with the levels of a column spread over threads: the plan (ksed1 / nstep) and the flux of the
// level above go through the communicator
template <class Comm>
__device__ __forceinline__ void th_sediment_comm(Comm &x, int nz, float dt, float dzq, ThHand &h,
                               float &pptrain, float &pptsnow, float &pptgraul, float &pptice)
{
    const float R1 = TH_R1, R2 = TH_R2;
    const int kts = 0, kte = nz - 1, k = x.k;
    const bool active = x.active;
    float vtrk = h.vtrk, vtnrk = h.vtnrk, vtik = h.vtik, vtnik = h.vtnik, vtsk = h.vtsk, vtgk = h.vtgk;
    float rr = h.rr, nr = h.nr, ri = h.ri, ni = h.ni, rs = h.rs, rg = h.rg;
    float qrten = h.qrten, nrten = h.nrten, qiten = h.qiten, niten = h.niten, qsten = h.qsten, qgten = h.qgten;
    const float rho = h.rho;
    float odzq, orho;
    float onstep[4]; int ksed1[4], nstep[4];
    int nblk[4];                                   /* the block's longest loop of each species (a by-product of the plan's exchange) */
    x.plan4(h.c4, h.ns4, kte, ksed1, onstep, nblk);

    /* ---- :2660-2770 sedimentation.  The four species fall independently of each other (each updates only its own
     * mass / number / tendency / surface flux), so their sub-step loops run as ONE loop of max(nstep) iterations with
     * one neighbour exchange (the six fluxes of the level above) per iteration; species s takes part while
     * n <= nstep(s), exactly as in its own loop (:2660-2770). ---- */
    odzq = 1.f / dzq; orho = 1.f / rho;
    int nall = 0;
    for (int s = 0; s < 4; ++s) { nstep[s] = (int)lroundf(1.f / onstep[s]); nall = nstep[s] > nall ? nstep[s] : nall; }
    (void)nall;
    /* a species that has finished everywhere in the block leaves the neighbour exchange (rain usually runs 2-5 times longer than the others) */
    const int nmax = imax(imax(nblk[0], nblk[1]), imax(nblk[2], nblk[3]));
    for (int n_ = 1; n_ <= nmax; ++n_) {
        float sed[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, up[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const unsigned slots = (n_ <= nblk[0] ? 3u : 0u) | (n_ <= nblk[1] ? 12u : 0u) | (n_ <= nblk[2] ? 16u : 0u) | (n_ <= nblk[3] ? 32u : 0u);
        if (slots & 3u) { sed[0] = active ? vtrk * rr : 0.f; sed[1] = active ? vtnrk * nr : 0.f; }
        if (slots & 12u) { sed[2] = active ? vtik * ri : 0.f; sed[3] = active ? vtnik * ni : 0.f; }
        if (slots & 16u) sed[4] = active ? vtsk * rs : 0.f;
        if (slots & 32u) sed[5] = active ? vtgk * rg : 0.f;
        x.up6_of(sed, up, slots);
        if (n_ <= nstep[0]) {
            const float sed_r = sed[0], sed_n = sed[1], up_r = up[0], up_n = up[1];
            if (active && k == kte) {
                qrten = qrten - sed_r * odzq * onstep[0] * orho;
                nrten = nrten - sed_n * odzq * onstep[0] * orho;
                rr = fmaxf(R1, rr - sed_r * odzq * dt * onstep[0]);
                nr = fmaxf(R2, nr - sed_n * odzq * dt * onstep[0]);
            } else if (active && k <= ksed1[0]) {
                qrten = qrten + (up_r - sed_r) * odzq * onstep[0] * orho;
                nrten = nrten + (up_n - sed_n) * odzq * onstep[0] * orho;
                rr = fmaxf(R1, rr + (up_r - sed_r) * odzq * dt * onstep[0]);
                nr = fmaxf(R2, nr + (up_n - sed_n) * odzq * dt * onstep[0]);
            }
            if (k == kts && rr > R1 * 10.f) pptrain = pptrain + sed_r * dt * onstep[0];
        }
        if (n_ <= nstep[1]) {
            const float sed_i = sed[2], sed_n = sed[3], up_i = up[2], up_n = up[3];
            if (active && k == kte) {
                qiten = qiten - sed_i * odzq * onstep[1] * orho;
                niten = niten - sed_n * odzq * onstep[1] * orho;
                ri = fmaxf(R1, ri - sed_i * odzq * dt * onstep[1]);
                ni = fmaxf(R2, ni - sed_n * odzq * dt * onstep[1]);
            } else if (active && k <= ksed1[1]) {
                qiten = qiten + (up_i - sed_i) * odzq * onstep[1] * orho;
                niten = niten + (up_n - sed_n) * odzq * onstep[1] * orho;
                ri = fmaxf(R1, ri + (up_i - sed_i) * odzq * dt * onstep[1]);
                ni = fmaxf(R2, ni + (up_n - sed_n) * odzq * dt * onstep[1]);
            }
            if (k == kts && ri > R1 * 10.f) pptice = pptice + sed_i * dt * onstep[1];
        }
        if (n_ <= nstep[2]) {
            const float sed_s = sed[4], up_s = up[4];
            if (active && k == kte) {
                qsten = qsten - sed_s * odzq * onstep[2] * orho;
                rs = fmaxf(R1, rs - sed_s * odzq * dt * onstep[2]);
            } else if (active && k <= ksed1[2]) {
                qsten = qsten + (up_s - sed_s) * odzq * onstep[2] * orho;
                rs = fmaxf(R1, rs + (up_s - sed_s) * odzq * dt * onstep[2]);
            }
            if (k == kts && rs > R1 * 10.f) pptsnow = pptsnow + sed_s * dt * onstep[2];
        }
        if (n_ <= nstep[3]) {
            const float sed_g = sed[5], up_g = up[5];
            if (active && k == kte) {
                qgten = qgten - sed_g * odzq * onstep[3] * orho;
                rg = fmaxf(R1, rg - sed_g * odzq * dt * onstep[3]);
            } else if (active && k <= ksed1[3]) {
                qgten = qgten + (up_g - sed_g) * odzq * onstep[3] * orho;
                rg = fmaxf(R1, rg + (up_g - sed_g) * odzq * dt * onstep[3]);
            }
            if (k == kts && rg > R1 * 10.f) pptgraul = pptgraul + sed_g * dt * onstep[3];
        }
    }

    h.rr = rr; h.nr = nr; h.ri = ri; h.ni = ni; h.rs = rs; h.rg = rg;
    h.qrten = qrten; h.nrten = nrten; h.qiten = qiten; h.niten = niten; h.qsten = qsten; h.qgten = qgten;
}

// :2777-2842 instant melt / freeze and the update of the level's state from its tendencies
__device__ __forceinline__ void th_level_finish(const ThState *__restrict__ T, float dt, const ThHand &h,
                               float &qv1d, float &qc1d, float &qi1d, float &qr1d, float &qs1d, float &qg1d, float &ni1d,
                               float &nr1d, float &t1d)
{
    const DK K_ = d_consts();
    const float R1 = TH_R1, R2 = TH_R2, T_0 = TH_T_0, HGFR = TH_HGFR, lsub = TH_lsub, xm0i = TH_xm0i, D0r = TH_D0r;
    const float am_r = TH_am_r, am_i = TH_am_i, bm_i = TH_bm_i, mu_i = TH_mu_i, mu_r = T->mu_r;
    const float *cie = T->cie, *cig = T->cig, *crg = T->crg;
    const float odt = 1.f / dt;
    float qrten = h.qrten, nrten = h.nrten, qiten = h.qiten, niten = h.niten, qsten = h.qsten, qgten = h.qgten;
    float qcten = h.qcten, qvten = h.qvten, tten = h.tten;
    const float rho = h.rho, temp = h.temp, ocp = h.ocp, lvap = h.lvap;
    float xri, xrc, lfus2, xDi, mvd_r;
    double lami, ilami, lamr;
    /* ---- :2777-2794 instant melt / freeze ---- */
    {
        xri = fmaxf(0.0f, qi1d + qiten * dt);
        if ((temp > T_0) && (xri > 0.0f)) {
            qcten = qcten + xri * odt;
            qiten = qiten - xri * odt;
            niten = -ni1d * odt;
            tten = tten - TH_lfus * ocp * xri * odt * 1;
        }
        xrc = fmaxf(0.0f, qc1d + qcten * dt);
        if ((temp < HGFR) && (xrc > 0.0f)) {
            lfus2 = lsub - lvap;
            qiten = qiten + xrc * odt;
            niten = niten + xrc / xm0i * odt;
            qcten = qcten - xrc * odt;
            tten = tten + lfus2 * ocp * xrc * odt * 1;
        }
        }
    /* ---- :2800-2842 apply ---- */
    {
        t1d = t1d + tten * dt;
        qv1d = fmaxf(1.E-10f, qv1d + qvten * dt);
        qc1d = qc1d + qcten * dt;
        if (qc1d <= R1) qc1d = 0.0f;
        qi1d = qi1d + qiten * dt;
        ni1d = fmaxf(R2 / rho, ni1d + niten * dt);
        if (qi1d <= R1) { qi1d = 0.0f; ni1d = 0.0f; }
        else {
            lami = d_powf(am_i * cig[1] * T->oig1 * ni1d / qi1d, T->obmi);
            ilami = 1. / lami;
            xDi = (float)((double)(bm_i + mu_i + 1.f) * ilami);
            if (xDi < 20.E-6f) lami = cie[1] / 20.E-6f;
            else if (xDi > 300.E-6f) lami = cie[1] / 300.E-6f;
            ni1d = (float)fmin((double)(cig[0] * T->oig2 * qi1d / am_i) * (lami * lami * lami), 250.e3 / (double)rho);
        }
        qr1d = qr1d + qrten * dt;
        nr1d = fmaxf(R2 / rho, nr1d + nrten * dt);
        if (qr1d <= R1) { qr1d = 0.0f; nr1d = 0.0f; }
        else {
            lamr = d_powf(am_r * crg[2] * T->org2 * nr1d / qr1d, T->obmr);
            mvd_r = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r > 2.5E-3f) mvd_r = 2.5E-3f;
            else if (mvd_r < D0r * 0.75f) mvd_r = D0r * 0.75f;
            lamr = (3.0f + mu_r + 0.672f) / mvd_r;
            nr1d = (float)((double)(crg[1] * T->org3 * qr1d) * (lamr * lamr * lamr) / (double)am_r);
        }
        qs1d = qs1d + qsten * dt;
        if (qs1d <= R1) qs1d = 0.0f;
        qg1d = qg1d + qgten * dt;
        if (qg1d <= R1) qg1d = 0.0f;
        }
}

// the three parts in sequence for the kernels with one level per thread (WaveComm / BlockComm)
template <class Comm>
__device__ __forceinline__ void th_column_lane(const ThState *__restrict__ T, Comm &x, int nz, float dt, float dzq,
                               float &qv1d, float &qc1d, float &qi1d, float &qr1d, float &qs1d, float &qg1d, float &ni1d,
                               float &nr1d, float &t1d, float p1d,
                               float &pptrain, float &pptsnow, float &pptgraul, float &pptice)
{
    ThHand h;
    if (!th_level_physics(T, x, nz, dt, dzq, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, t1d, p1d, h)) return;
    th_sediment_comm(x, nz, dt, dzq, h, pptrain, pptsnow, pptgraul, pptice);
    th_level_finish(T, dt, h, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, t1d);
}

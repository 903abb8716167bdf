// icar_amd/csrc/nsas_column.h -- one column of the NSAS convection scheme as cu_driver.f90 calls it (convection = kCU_NSAS = 4): the
// per-row body of cu_nsas, the deep scheme nsas2d and the shallow scheme nscv2d.  Plain C that a C compiler (tests/support/nsas_oracle.c,
// the host restatement) and hipcc (cu_nsas.hip) both accept.
//
// Reference algorithm: src/physics/cu_nsas.f90 -- cu_nsas :158-305, nsas2d :552-2081, fpvs :2083-2123, nscv2d :2339-3288, with the
// arguments of src/physics/cu_driver.f90:354-417: itimestep = STEPCU = 1, mp_physics = 5 so ncloud = 2 (:141-147), pgcon absent so 0.55
// (:149-156), the levels kts .. kte-1 (n below), cp = 1012, cliq = 4190, cpv = 4*461.6, g = 9.81, xlv = 2.5E6, r_d = 287, r_v = 461.6,
// ep_1 = EP1 = 461.5/287.058 - 1 (icar_constants.f90:391-392, 419), cice = 2106, xls = 2.85E6, psat = 610.78, dx_factor_nsas = 1 when
// dx <= 1000 and 2 otherwise, w = w_real, hfx = sensible_heat, qfx = latent_heat / 2260000.  REAL(4) in the reference's operation order
// (every expression below is the reference's text; C and Fortran give * / and + - the same precedence and associate them to the left),
// no contraction, IEEE division and square root.  exp, pow and sqrt are the includer's: NSAS_EXPF, NSAS_POWF, NSAS_SQRTF (libm on the
// host; the device's gf_expf / gf_powf are held to libm bit for bit elsewhere).
//
// Powers, read off the LLVM IR that flang -O2 makes of cu_nsas.f90: to**2, tem**2, t1**2, dt**2, vshear**2 and the two squares under
// the shear's sqrt are x*x; tem**3 and vshear**3 are (x*x)*x (llvm.powi with a constant exponent, expanded so); beta**tem (:1297),
// ptem**h1 (:3126) and fpvs's tr**xa / tr**xai are calls of powf; exp is expf and sqrt the IEEE instruction.
//
// fpvs.  Its constants arrive as run-time arguments, so the compiled reference makes them in REAL(4) in the order written:
// ttp = t0c + 0.01, xa = -(cvap - cliq)/rv, xb = xa + hvap/(rv*ttp), xai = -(cvap - cice)/rv, xbi = xai + hsub/(rv*ttp); nsas_fpvs
// does the same arithmetic on the same REAL(4) values, which gives the same bits whether or not a compiler folds it.  The reference
// evaluates the formula with tr = ttp/t and then again with tr = ttp/180 (t < 180) or ttp/330 (t >= 330), the arm (ice below ttp)
// chosen by t itself each time; only the last value is kept, so one evaluation with the final tr gives the same bits.
//
// Values shared along a row.  In nsas2d kbmax, kbm and kmax are scalars made from all the columns its..ite of the row (:619-632): the
// last k at which any column passes the pressure test, i.e. the maximum over the columns of each column's own last k, then min(., kte).
// nsas_row_limits makes a column's own three values; the caller takes the maxima along the row and hands them to nsas_deep.  In nscv2d
// kbm and kmax are per column (:2424-2438) and made inside nsas_shallow.
//
// Early returns.  `if(totflg) return` leaves nsas2d (:778, :820, :987, :1021, :1130, :1443, :1893 and the end) and nscv2d (:2388,
// :2625, :2674, :2784, :2886 and the end) once no column of the row convects.  A column leaves here as soon as its own cnvflg falls.
// That gives the same bits because every statement after the first possible return that writes an argument of the routine (rain,
// kbot, ktop, icps, t1, q1, u1, v1, qc2, qi2) is guarded by cnvflg(i):
//   nsas2d  t1/q1/u1/v1 :1933-1937 (cnvflg and k <= ktcon), :2019-2021 (cnvflg and flg), :2052-2055 (cnvflg and rain <= 0);
//           rain :1998 :2021 :2038-2040, kbot/ktop/icps :2042-2044 (all under cnvflg); qi2/qc2 :2070-2073 (cnvflg and rain > 0).
//   nscv2d  kbot/ktop :2370-2371 and rain = 0 :2373 stand BEFORE the first return; t1/q1/u1/v1 :3158-3162, rain :3215 (cnvflg);
//           :3218-3251 is guarded by flg(i), which :3192 makes equal to cnvflg(i) and which only falls afterwards; :3258-3261, qi2/qc2
//           :3276-3279 (cnvflg).
// The statements that are NOT guarded by cnvflg all write locals that no guarded statement of another column reads: zi and xlamb
// :822-832, kbdtr and beta :1289-1291, qrcdo / qrcd :1308-1309, xpwev :1729, acrt :1820, acrtfct and w1..w4 :1837-1847, the sums
// :1916-1922 and :1964-1967, delq / deltv / qevap :1990-1992 in nsas2d; kbm / kmax / zi / xlamue / kpbl :2424-2478, kbcon1 :2751,
// ktcon1 :2900, the sums :3145-3150 :3189-3192 and deltv / delq / qevap :3210-3212 in nscv2d.
// tests/golden/make_golden_nsas.py asserts the consequence on the compiled reference: single columns of a flat row computed alone
// have the bits they have in the row.
//
// Not built, because no evaluated statement that reaches a result reads it:
//   tend%u / tend%v (rucuten / rvcuten).  cu_driver.f90:502-507 applies neither.  The updated u1 / v1 could only matter through the
//   shallow scheme's uo / vo (:2497-2498, vshear -> edt -> evaporation).  nscv2d skips a column with icps = 1 (:2367), icps = 1 is set
//   only where nsas2d ends with cnvflg and rain > 0 (:2039-2044); a column that ends with cnvflg and rain <= 0 gets u1 = uo, v1 = vo
//   back at :2054-2055, where uo / vo were restored to u1 / v1 at :1902-1903 before the feedback; and a column whose cnvflg fell never
//   reaches :1936.  So every column nscv2d works on carries the model's own u, v, and the shallow u1 / v1 of :3161-3162 are read by
//   nothing.  With them go ucko, vcko, ucdo, vcdo, dellau, dellav, delubar, delvbar.
//   tvo, delhbar / delqbar / deltbar, delq / deltv, the update of dellaq by the evaporation (:2026, :3248), kbdtr, klcl, ktdown, kbds,
//   adet, aatmp, excess, plcl, vmax, thx above level 1, qrski, wstar as an array: written and never read (or read only by these).
//   ncloud < 2 arms (mp_physics = 5).
//
// Elements an evaluated statement can read.  nsas2d initialises its level arrays up to the row's kmax only, zi from 2 to kte, and
// never zi(1) or zi(kte+1).  Every read is of an element written before: a convecting column has kbcon <= kbmax and kbcon /= kmax, and
// kbmax <= kmax <= kte, so kbcon <= kte-1; ktcon <= kmax-1 after the swap of :1205-1211; jmin < ktcon.  zi(k+2) is read with
// k < kbcon (:893, :1282, :1321) or k < jmin (:1317, :1352, :1382, :1744, :1767), at most zi(kte); zi(ktcon+1) and zi(kb+1) (:1259) at most
// zi(kte); zi(3) - zi(2) at :910 is reached only with kbcon < kmax <= kte, kbcon > kb >= 1, so kte >= 3 there (with two scheme levels
// every column leaves at :771 and at :2617 and nothing is read out of bounds; with one, nscv2d's unguarded xlamue(i,kte) =
// xlamue(i,km1) at :2456 reads xlamue(i,0): NSAS_MIN_LEVELS = 2).  zl(k+1) is read with k < ktcon or k < kmax.  In nscv2d kmax(i) = k+1 is NOT cut to
// kte (:2432): a column whose top level lies above 0.6 of its surface pressure has kmax = kte+1, and then kbcon / ktcon may reach kte
// and del(kte+1) / zi(kte+1) be read: a model top below about 4 km, where the reference itself reads past its automatic arrays; here
// such a read stays inside the workspace (nl >= n + 2 and zi is not the last array).  The bounds program
// tests/support/nsas_bounds_main.c runs this file under the address and undefined-behaviour sanitizers at every level count, every
// level array an allocation of the reference's own extent, filled with two different patterns.
//
// The level arrays of a column live in a workspace laid out [array][level][column]: NSAS_WS(a, k) is level k (1-based, 1 = lowest)
// of array a; `stride` is the number of columns the workspace holds (1 on the host), `nl` its level count (>= n + 2).
#pragma once
#include <stddef.h>

#ifndef NSAS_FN
#define NSAS_FN static inline
#endif

enum { NSAS_DEL = 0, NSAS_ZL, NSAS_PRSL, NSAS_T1, NSAS_Q1, NSAS_QC2, NSAS_QI2,                       /* cu_nsas's row arrays */
       NSAS_P, NSAS_TO, NSAS_QO, NSAS_UO, NSAS_VO, NSAS_QESO, NSAS_HEO, NSAS_HESO, NSAS_DBYO, NSAS_FRH, NSAS_FENT1, NSAS_FENT2,
       NSAS_XLAMB, NSAS_ETA, NSAS_ETAD, NSAS_HCKO, NSAS_QCKO, NSAS_HCDO, NSAS_QCDO, NSAS_QRCDO, NSAS_PWO, NSAS_PWDO, NSAS_DELLAL,
       NSAS_DELLAH, NSAS_DELLAQ, NSAS_XHCD, NSAS_XQCD, NSAS_ZI, NSAS_PO, NSAS_NARR };
#define NSAS_MIN_LEVELS 2           /* of the scheme (kte - 1 of the model): with one, :2456 reads xlamue(i,0) */
#define NSAS_MAX_LEVELS 128         /* of the scheme; sizes the workspace */

/* what the coverage conditions of tests/test_nsas_oracle.py count (host only: NSAS_DIAG) */
enum { NSAS_D_DEEP_RAIN = 1, NSAS_D_SHALLOW = 2, NSAS_D_DOWNDRAFT = 4, NSAS_D_EVAP = 8, NSAS_D_EVAP_CUT = 16, NSAS_D_RESTORED = 32,
       NSAS_D_ICE_ONLY = 64, NSAS_D_WATER_ONLY = 128, NSAS_D_MIXED = 256, NSAS_D_FPVS_ICE = 512, NSAS_D_FPVS_WATER = 1024,
       NSAS_D_FPVS_COLD = 2048, NSAS_D_FPVS_HOT = 4096, NSAS_D_SFLX_NEG = 8192, NSAS_D_NO_KBCON = 16384, NSAS_D_PBCDIF = 32768,
       NSAS_D_DRY = 65536, NSAS_D_THIN = 131072, NSAS_D_LAND = 262144, NSAS_D_WATER = 524288, NSAS_D_DXF1 = 1048576,
       NSAS_D_DXF2 = 2097152, NSAS_D_SHALLOW_EVAP = 4194304, NSAS_D_DEEP_END = 8388608 };
#ifdef NSAS_DIAG
#define NSAS_FLAG(x) (*diag |= (x))
#else
#define NSAS_FLAG(x) ((void)0)
#endif

/* Fortran's max / min as this flang lowers them: a compare and a select of the first operand */
#define NSAS_MAX(a, b) ((a) > (b) ? (a) : (b))
#define NSAS_MIN(a, b) ((a) < (b) ? (a) : (b))

/* cu_driver.f90:401-412 */
#define NSAS_CP 1012.0f
#define NSAS_CLIQ 4190.f
#define NSAS_CVAP (4.f * 461.6f)
#define NSAS_G 9.81f
#define NSAS_HVAP 2.5E6f
#define NSAS_RD 287.f
#define NSAS_RV 461.6f
#define NSAS_FV (461.5f / 287.058f - 1.f)
#define NSAS_CICE 2106.f
#define NSAS_XLS 2.85E6f
#define NSAS_PSAT 610.78f
#define NSAS_PGCON 0.55f
#define NSAS_T0C 273.15f
#define NSAS_QMIN 1.0e-30f

/* the model's arrays of one column: element k (0-based from the ground) of an array sits at [k * ls]; pint and w have n + 1 levels */
typedef struct {
    const float *t, *qv, *qc, *qi, *pi, *rho, *w, *dz, *p, *pint, *u, *v;
    size_t ls;
} NsasIn;

/* what cu_nsas carries from nsas2d to nscv2d and to its own end, per column */
typedef struct {
    float rain1, rain2;
    int kbot, ktop, icps;
} NsasOut;

#ifndef NSAS_WS                     /* the bounds program puts an accessor here that knows the reference's extents */
#define NSAS_WS(a, k) ws[((size_t)(a) * nl + (size_t)(k)) * stride]
#endif

NSAS_FN float nsas_fpvs(float t, int *diag)                                          /* :2083-2123 with ice = 1 */
{
    (void)diag;
    const float ttp = NSAS_T0C + 0.01f;
    const float dldt = NSAS_CVAP - NSAS_CLIQ;
    const float xa = -dldt / NSAS_RV;
    const float xb = xa + NSAS_HVAP / (NSAS_RV * ttp);
    const float dldti = NSAS_CVAP - NSAS_CICE;
    const float xai = -dldti / NSAS_RV;
    const float xbi = xai + NSAS_XLS / (NSAS_RV * ttp);
    float tr = ttp / t;
    if (t < 180.f) { tr = ttp / 180.f; NSAS_FLAG(NSAS_D_FPVS_COLD); }
    if (t >= 330.f) { tr = ttp / 330.f; NSAS_FLAG(NSAS_D_FPVS_HOT); }
    if (t < ttp) { NSAS_FLAG(NSAS_D_FPVS_ICE); return NSAS_PSAT * NSAS_POWF(tr, xai) * NSAS_EXPF(xbi * (1.f - tr)); }
    NSAS_FLAG(NSAS_D_FPVS_WATER);
    return NSAS_PSAT * NSAS_POWF(tr, xa) * NSAS_EXPF(xb * (1.f - tr));
}

/* a column's own kbmax, kbm, kmax of :619-628 before the min with kte: the caller takes the row's maxima, then min(., n) (:629-632) */
NSAS_FN void nsas_row_limits(NsasIn in, int n, int *kbmax, int *kbm, int *kmax)
{
    const float ps = in.pint[0] * 0.001f;
    *kbmax = *kbm = *kmax = n;
    for (int k = 1; k <= n; k++) {
        const float prsl = in.p[(size_t)(k - 1) * in.ls] * 0.001f;
        if (prsl > ps * 0.45f) *kbmax = k + 1;
        if (prsl > ps * 0.70f) *kbm = k + 1;
        if (prsl > ps * 0.04f) *kmax = k + 1;
    }
}

#define DEL(k) NSAS_WS(NSAS_DEL, k)
#define ZL(k) NSAS_WS(NSAS_ZL, k)
#define PRSL(k) NSAS_WS(NSAS_PRSL, k)
#define T1(k) NSAS_WS(NSAS_T1, k)
#define Q1(k) NSAS_WS(NSAS_Q1, k)
#define QC2(k) NSAS_WS(NSAS_QC2, k)
#define QI2(k) NSAS_WS(NSAS_QI2, k)
#define P(k) NSAS_WS(NSAS_P, k)
#define TO(k) NSAS_WS(NSAS_TO, k)
#define QO(k) NSAS_WS(NSAS_QO, k)
#define UO(k) NSAS_WS(NSAS_UO, k)
#define VO(k) NSAS_WS(NSAS_VO, k)
#define QESO(k) NSAS_WS(NSAS_QESO, k)
#define HEO(k) NSAS_WS(NSAS_HEO, k)
#define HESO(k) NSAS_WS(NSAS_HESO, k)
#define DBYO(k) NSAS_WS(NSAS_DBYO, k)
#define FRH(k) NSAS_WS(NSAS_FRH, k)
#define FENT1(k) NSAS_WS(NSAS_FENT1, k)
#define FENT2(k) NSAS_WS(NSAS_FENT2, k)
#define XLAMB(k) NSAS_WS(NSAS_XLAMB, k)
#define ETA(k) NSAS_WS(NSAS_ETA, k)
#define ETAD(k) NSAS_WS(NSAS_ETAD, k)
#define HCKO(k) NSAS_WS(NSAS_HCKO, k)
#define QCKO(k) NSAS_WS(NSAS_QCKO, k)
#define HCDO(k) NSAS_WS(NSAS_HCDO, k)
#define QCDO(k) NSAS_WS(NSAS_QCDO, k)
#define QRCDO(k) NSAS_WS(NSAS_QRCDO, k)
#define PWO(k) NSAS_WS(NSAS_PWO, k)
#define PWDO(k) NSAS_WS(NSAS_PWDO, k)
#define DELLAL(k) NSAS_WS(NSAS_DELLAL, k)
#define DELLAH(k) NSAS_WS(NSAS_DELLAH, k)
#define DELLAQ(k) NSAS_WS(NSAS_DELLAQ, k)
#define XHCD(k) NSAS_WS(NSAS_XHCD, k)
#define XQCD(k) NSAS_WS(NSAS_XQCD, k)
#define ZI(k) NSAS_WS(NSAS_ZI, k)
#define PO(k) NSAS_WS(NSAS_PO, k)

/* cu_nsas :169-209: the row arrays of one column.  dot is made where it is read (nsas_dot). */
NSAS_FN void nsas_setup(NsasIn in, int n, float *ws, size_t stride, size_t nl)
{
    float zii = 0.0f;
    for (int k = 1; k <= n; k++) {
        const size_t a = (size_t)(k - 1) * in.ls;
        const float prsll = in.p[a] * 0.001f;
        const float zii1 = zii + in.dz[a];
        PRSL(k) = prsll;
        ZL(k) = 0.5f * (zii + zii1);
        zii = zii1;
        DEL(k) = prsll * NSAS_G / NSAS_RD * in.dz[a] / in.t[a];
        Q1(k) = in.qv[a];
        T1(k) = in.t[a];
        QI2(k) = in.qi[a];
        QC2(k) = in.qc[a];
    }
}

NSAS_FN float nsas_dot(NsasIn in, int k)                                              /* :172 */
{
    return -5.0e-4f * NSAS_G * in.rho[(size_t)(k - 1) * in.ls] * (in.w[(size_t)(k - 1) * in.ls] + in.w[(size_t)k * in.ls]);
}

/* qeso of :678-680 and its repeats: 0.01 fpvs, the mixing ratio at pressure pp, the floor */
NSAS_FN float nsas_qes(float t, float pp, float eps, float floor_, int *diag)
{
    float q = 0.01f * nsas_fpvs(t, diag);
    q = eps * q / (pp + (eps - 1.f) * q);
    return NSAS_MAX(q, floor_);
}

/* nsas2d :552-2081 for one column.  kbmax, kbm, kmax: the row's (nsas_row_limits).  slimsk = xland.  Updates T1, Q1, QC2, QI2. */
NSAS_FN void nsas_deep(NsasIn in, int n, int kbmax, int kbm, int kmax, float slimsk, float delt, float delx, int dx_factor_nsas,
                       float *ws, size_t stride, size_t nl, NsasOut *o, int *diag)
{
    const float alphal = 0.5f, betal = 0.05f, betas = 0.05f, c0 = 0.002f, c1 = 0.002f, xlamdd = 1.0e-4f, xlamde = 1.0e-4f;
    const float clam = 0.1f, cxlamu = 1.0e-4f, aafac = 0.1f, dthk = 25.f, cincrmax = 180.f, cincrmin = 120.f, mbdt = 10.f;
    const float edtmaxl = 0.3f, edtmaxs = 0.3f, evfacts = 0.3f, evfactl = 0.3f;
    const float tf = 233.16f, tcr = 263.16f, tcrf = 1.0f / (tcr - tf);
    const float pcrit[15] = { 850.f, 800.f, 750.f, 700.f, 650.f, 600.f, 550.f, 500.f, 450.f, 400.f, 350.f, 300.f, 250.f, 200.f, 150.f };
    const float acritt[15] = { .0633f, .0445f, .0553f, .0664f, .075f, .1082f, .1521f, .2216f, .3151f, .3677f, .41f, .5255f, .7663f, 1.1686f, 1.6851f };
    const float pgcon = NSAS_PGCON, g_ = NSAS_G, cp_ = NSAS_CP, hvap_ = NSAS_HVAP, rv_ = NSAS_RV, rd_ = NSAS_RD, fv_ = NSAS_FV;
    const float qmin_ = NSAS_QMIN, t0c_ = NSAS_T0C;
    const float el2orc = hvap_ * hvap_ / (rv_ * cp_);
    const float eps = rd_ / rv_;
    const float fact1 = (NSAS_CVAP - NSAS_CLIQ) / rv_;
    const float fact2 = hvap_ / rv_ - fact1 * t0c_;
    const int kmax1 = kmax - 1, kte1 = n - 1;
    const float dt2 = delt;
    const float dtmin = NSAS_MAX(dt2, 1200.f), dtmax = NSAS_MAX(dt2, 3600.f);
    float W1l, W2l, W3l, W4l, W1s, W2s, W3s, W4s, w1, w2, w3, w4;
    float dz, dp, es, pprime, qs, dqsdp, desdt, dqsdt, gamma, dt, dq, po, tem, tem1, factor, ptem, dz1, qrch, etah, qlk, qc, rfact;
    float shear, e1, dh, dhh, dg, aup, adw, dellat, xdby, xqrch, xpw, xpwd, evef, cincr, beta, edtmax, qcirs, qrcd, dv1, dv2, dv3, dv1q,
          dv2q, dv3q, ptem1, dvq1;
    float hmax, hkbo, qkbo, pdot, pbcdif, xlamud, pwavo, aa1, aa2, hmin, xmbmax, qlko_ktcon = 0.0f, vshear, edt, edto, edtx, sumx, xlamd,
          pwevo, xaa0, xpwav, xpwev, acrt, acrtfct, dtconv, f, xk, xmb, rntot, delqev, delq2, qcond, qevap, rain;
    int kb, kbcon, kbcon1, ktcon, ktcon1, lmin, jmin, flg, k, indx, kk;
    (void)alphal; (void)kte1; (void)dv2; (void)dv2q;

    if (dx_factor_nsas == 1) {                                                        /* :567-586 */
        const float dx_factor = 250.f / delx;
        W1l = dx_factor * 0.1f * (-1.f);
        W2l = dx_factor * (-1.f);
        W3l = dx_factor * (-1.f);
        W4l = dx_factor * 0.1f * (-1.f);
        W1s = W1l; W2s = W2l; W3s = W3l; W4s = W4l;
        NSAS_FLAG(NSAS_D_DXF1);
    } else {
        W1l = -8.E-3f; W2l = -4.E-2f; W3l = -5.E-3f; W4l = -5.E-4f;
        W1s = -2.E-4f; W2s = -2.E-3f; W3s = -1.E-3f; W4s = -2.E-5f;
        NSAS_FLAG(NSAS_D_DXF2);
    }
    NSAS_FLAG(slimsk == 1.f ? NSAS_D_LAND : NSAS_D_WATER);
    o->rain1 = 0.0f; o->kbot = n + 1; o->ktop = 0; o->icps = 0;                       /* :592-595 */
    rain = 0.0f; edto = 0.0f; edtx = 0.0f; edt = 0.0f; jmin = 1; lmin = 1;

    for (k = 1; k <= n; k++) {                                                        /* :636-646 */
        PWO(k) = 0.0f; PWDO(k) = 0.0f; DELLAL(k) = 0.0f; HCKO(k) = 0.0f; QCKO(k) = 0.0f; HCDO(k) = 0.0f; QCDO(k) = 0.0f;
    }
    for (k = 1; k <= kmax; k++) {                                                     /* :648-666 */
        P(k) = PRSL(k) * 10.f;
        TO(k) = T1(k); QO(k) = Q1(k);
        DBYO(k) = 0.0f; FENT1(k) = 1.0f; FENT2(k) = 1.0f; FRH(k) = 0.0f;
        UO(k) = in.u[(size_t)(k - 1) * in.ls]; VO(k) = in.v[(size_t)(k - 1) * in.ls];
    }
    for (k = 1; k <= kmax; k++) {                                                     /* :676-693 */
        QESO(k) = nsas_qes(TO(k), P(k), eps, qmin_, diag);
        QO(k) = NSAS_MAX(QO(k), 1.e-10f);
        HEO(k) = g_ * ZL(k) + cp_ * TO(k) + hvap_ * QO(k);
        HESO(k) = g_ * ZL(k) + cp_ * TO(k) + hvap_ * QESO(k);
    }
    hmax = HEO(1); kb = 1;                                                            /* :698-710 */
    for (k = 2; k <= kbm; k++) if (HEO(k) > hmax) { kb = k; hmax = HEO(k); }
    for (k = 1; k <= kmax1; k++) {                                                    /* :712-742 */
        dz = .5f * (ZL(k+1) - ZL(k));
        dp = .5f * (P(k+1) - P(k));
        es = 0.01f * nsas_fpvs(TO(k+1), diag);
        pprime = P(k+1) + (eps - 1.f) * es;
        qs = eps * es / pprime;
        dqsdp = -qs / pprime;
        desdt = es * (fact1 / TO(k+1) + fact2 / (TO(k+1) * TO(k+1)));
        dqsdt = qs * P(k+1) * desdt / (es * pprime);
        gamma = el2orc * QESO(k+1) / (TO(k+1) * TO(k+1));
        dt = (g_ * dz + hvap_ * dqsdp * dp) / (cp_ * (1.f + gamma));
        dq = dqsdt * dt + dqsdp * dp;
        TO(k) = TO(k+1) + dt;
        QO(k) = QO(k+1) + dq;
        po = .5f * (P(k) + P(k+1));
        QESO(k) = nsas_qes(TO(k), po, eps, qmin_, diag);
        QO(k) = NSAS_MAX(QO(k), 1.e-10f);
        FRH(k) = 1.f - NSAS_MIN(QO(k) / QESO(k), 1.f);
        HEO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QO(k);
        HESO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QESO(k);
        UO(k) = .5f * (UO(k) + UO(k+1));
        VO(k) = .5f * (VO(k) + VO(k+1));
    }
    hkbo = HEO(kb); qkbo = QO(kb);                                                    /* :746-772 */
    flg = 1; kbcon = kmax;
    for (k = 1; k <= kbmax; k++)
        if (flg && k > kb) {
            if (hkbo > HESO(k)) { flg = 0; kbcon = k; }
        }
    if (kbcon == kmax) { NSAS_FLAG(NSAS_D_NO_KBCON); return; }

    pdot = 10.f * nsas_dot(in, kbcon);                                                /* :780-813 */
    if (slimsk == 1.f) { w1 = W1l; w2 = W2l; w3 = W3l; w4 = W4l; } else { w1 = W1s; w2 = W2s; w3 = W3s; w4 = W4s; }
    if (pdot <= w4) tem = (pdot - w4) / (w3 - w4);
    else if (pdot >= -w4) tem = -(pdot + w4) / (w4 - w3);
    else tem = 0.f;
    tem = NSAS_MAX(tem, -1.f);
    tem = NSAS_MIN(tem, 1.f);
    tem = 1.f - tem;
    tem1 = .5f * (cincrmax - cincrmin);
    cincr = cincrmax - tem * tem1;
    pbcdif = -P(kbcon) + P(kb);
    if (pbcdif > cincr) { NSAS_FLAG(NSAS_D_PBCDIF); return; }

    for (k = 2; k <= n; k++) ZI(k) = 0.5f * (ZL(k-1) + ZL(k));                        /* :822-832 */
    for (k = 1; k <= n - 1; k++) XLAMB(k) = clam / ZI(k+1);
    for (k = 2; k <= kmax1; k++) if (k > kbcon) XLAMB(k) = XLAMB(kbcon);              /* :837-843 */
    xlamud = XLAMB(kbcon);                                                            /* :850 */
    for (k = 2; k <= kmax1; k++)                                                      /* :857-865 */
        if (k > kbcon) {
            tem = QESO(k) / QESO(kbcon);
            FENT1(k) = tem * tem;
            FENT2(k) = tem * tem * tem;
        }
    for (k = 2; k <= kmax1; k++)                                                      /* :871-878 */
        if (k >= kbcon) {
            tem = cxlamu * FRH(k) * FENT2(k);
            XLAMB(k) = XLAMB(k) * FENT1(k) + tem;
        }
    for (k = 1; k <= n; k++) ETA(k) = 1.f;                                            /* :882-888 */
    for (k = kbmax; k >= 2; k--)                                                      /* :890-898 */
        if (k < kbcon && k >= kb) {
            dz = ZI(k+2) - ZI(k+1);
            ptem = 0.5f * (XLAMB(k) + XLAMB(k+1)) - xlamud;
            ETA(k) = ETA(k+1) / (1.f + ptem * dz);
        }
    for (k = 2; k <= kmax1; k++)                                                      /* :899-907 */
        if (k > kbcon) {
            dz = ZI(k+1) - ZI(k);
            ptem = 0.5f * (XLAMB(k) + XLAMB(k-1)) - xlamud;
            ETA(k) = ETA(k-1) * (1.f + ptem * dz);
        }
    dz = ZI(3) - ZI(2);                                                               /* :908-914 */
    ptem = 0.5f * (XLAMB(1) + XLAMB(2)) - xlamud;
    ETA(1) = ETA(2) / (1.f + ptem * dz);

    HCKO(kb) = hkbo; QCKO(kb) = qkbo; pwavo = 0.f;                                    /* :918-927 */
    for (k = 2; k <= kmax1; k++)                                                      /* :931-949 */
        if (k > kb) {
            dz = ZI(k+1) - ZI(k);
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            HCKO(k) = ((1.f - tem1) * HCKO(k-1) + tem * 0.5f * (HEO(k) + HEO(k-1))) / factor;
            DBYO(k) = HCKO(k) - HESO(k);
        }
    flg = 1; kbcon1 = kmax;                                                           /* :954-981 */
    for (k = 2; k <= kmax; k++)
        if (flg && k >= kbcon && DBYO(k) > 0.f) { kbcon1 = k; flg = 0; }
    if (kbcon1 == kmax) return;
    tem = P(kbcon) - P(kbcon1);
    if (tem > dthk) { NSAS_FLAG(NSAS_D_DRY); return; }

    flg = 1; ktcon = 1;                                                               /* :993-1015 */
    for (k = 2; k <= kmax1; k++)
        if (DBYO(k) < 0.f && flg && k > kbcon1) { ktcon = k; flg = 0; }
    if ((P(kbcon) - P(ktcon)) < 150.f) { NSAS_FLAG(NSAS_D_THIN); return; }

    hmin = HEO(kbcon1); lmin = kbmax; jmin = kbmax;                                   /* :1026-1051 */
    for (k = 2; k <= kbmax; k++)
        if (k > kbcon1 && HEO(k) < hmin) { lmin = k + 1; hmin = HEO(k); }
    jmin = NSAS_MIN(lmin, ktcon - 1);
    jmin = NSAS_MAX(jmin, kbcon1 + 1);
    if (jmin >= ktcon) return;
    dp = 1000.f * DEL(kbcon);                                                         /* :1055-1061 */
    xmbmax = dp / (g_ * dt2);

    aa1 = 0.f;                                                                        /* :1066-1104 */
    for (k = 2; k <= kmax; k++)
        if (k > kb && k < ktcon) {
            dz = .5f * (ZL(k+1) - ZL(k-1));
            dz1 = (ZI(k+1) - ZI(k));
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz1;
            tem1 = 0.5f * xlamud * dz1;
            factor = 1.f + tem - tem1;
            QCKO(k) = ((1.f - tem1) * QCKO(k-1) + tem * 0.5f * (QO(k) + QO(k-1))) / factor;
            qcirs = ETA(k) * QCKO(k) - ETA(k) * qrch;
            if (qcirs > 0.f && k >= kbcon) {
                etah = .5f * (ETA(k) + ETA(k-1));
                if (k > jmin) {
                    dp = 1000.f * DEL(k);
                    qlk = qcirs / (ETA(k) + etah * (c0 + c1) * dz1);
                    DELLAL(k) = etah * c1 * dz1 * qlk * g_ / dp;
                } else {
                    qlk = qcirs / (ETA(k) + etah * c0 * dz1);
                }
                aa1 = aa1 - dz1 * g_ * qlk;
                qc = qlk + qrch;
                PWO(k) = etah * c0 * dz1 * qlk;
                QCKO(k) = qc;
                pwavo = pwavo + PWO(k);
            }
        }
    for (k = 2; k <= kmax; k++)                                                       /* :1108-1124 */
        if (k >= kbcon && k < ktcon) {
            dz1 = ZL(k+1) - ZL(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            rfact = 1.f + fv_ * cp_ * gamma * TO(k) / hvap_;
            aa1 = aa1 + dz1 * (g_ / (cp_ * TO(k))) * DBYO(k) / (1.f + gamma) * rfact;
            aa1 = aa1 + dz1 * g_ * fv_ * NSAS_MAX(0.f, (QESO(k) - QO(k)));
        }
    if (aa1 <= 0.f) return;

    aa2 = aafac * aa1;                                                                /* :1136-1163 */
    flg = 1; ktcon1 = kmax1;
    for (k = 2; k <= kmax; k++)
        if (flg) {
            if (k >= ktcon && k < kmax) {
                dz1 = ZL(k+1) - ZL(k);
                gamma = el2orc * QESO(k) / (TO(k) * TO(k));
                rfact = 1.f + fv_ * cp_ * gamma * TO(k) / hvap_;
                aa2 = aa2 + dz1 * (g_ / (cp_ * TO(k))) * DBYO(k) / (1.f + gamma) * rfact;
                if (aa2 < 0.f) { ktcon1 = k; flg = 0; }
            }
        }
    for (k = 2; k <= kmax; k++)                                                       /* :1168-1201 */
        if (k >= ktcon && k < ktcon1) {
            dz = (ZI(k+1) - ZI(k));
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            QCKO(k) = ((1.f - tem1) * QCKO(k-1) + tem * 0.5f * (QO(k) + QO(k-1))) / factor;
            qcirs = ETA(k) * QCKO(k) - ETA(k) * qrch;
            if (qcirs > 0.f) {
                etah = .5f * (ETA(k) + ETA(k-1));
                dp = 1000.f * DEL(k);
                qlk = qcirs / (ETA(k) + etah * (c0 + c1) * dz);
                DELLAL(k) = etah * c1 * dz * qlk * g_ / dp;
                qc = qlk + qrch;
                PWO(k) = etah * c0 * dz * qlk;
                QCKO(k) = qc;
                pwavo = pwavo + PWO(k);
            }
        }
    kk = ktcon; ktcon = ktcon1; ktcon1 = kk;                                          /* :1205-1211 */
    k = ktcon - 1;                                                                    /* :1219-1234 */
    gamma = el2orc * QESO(k) / (TO(k) * TO(k));
    qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
    dq = QCKO(k) - qrch;
    if (dq > 0.f) { qlko_ktcon = dq; QCKO(k) = qrch; }

    vshear = 0.f;                                                                     /* :1241-1269 */
    for (k = 2; k <= kmax; k++)
        if (k > kb && k <= ktcon) {
            shear = NSAS_SQRTF((UO(k) - UO(k-1)) * (UO(k) - UO(k-1)) + (VO(k) - VO(k-1)) * (VO(k) - VO(k-1)));
            vshear = vshear + shear;
        }
    vshear = 1.e3f * vshear / (ZI(ktcon+1) - ZI(kb+1));
    e1 = 1.591f - .639f * vshear + .0953f * (vshear * vshear) - .00496f * (vshear * vshear * vshear);
    edt = 1.f - e1;
    edt = NSAS_MIN(edt, .9f);
    edt = NSAS_MAX(edt, .0f);
    edto = edt; edtx = edt;

    sumx = 0.f;                                                                       /* :1273-1299 */
    for (k = 1; k <= kmax1; k++)
        if (k >= 1 && k < kbcon) { dz = ZI(k+2) - ZI(k+1); sumx = sumx + dz; }
    beta = betas;
    if (slimsk == 1.f) beta = betal;
    dz = (sumx + ZI(2)) / (float)kbcon;
    tem = 1.f / (float)kbcon;
    xlamd = (1.f - NSAS_POWF(beta, tem)) / dz;

    for (k = 1; k <= kmax; k++) { ETAD(k) = 1.f; QRCDO(k) = 0.f; }                    /* :1303-1311 */
    for (k = kmax1; k >= 1; k--) {                                                    /* :1313-1327 */
        if (k < jmin && k >= kbcon) {
            dz = (ZI(k+2) - ZI(k+1));
            ptem = xlamdd - xlamde;
            ETAD(k) = ETAD(k+1) * (1.f - ptem * dz);
        } else if (k < kbcon) {
            dz = (ZI(k+2) - ZI(k+1));
            ptem = xlamd + xlamdd - xlamde;
            ETAD(k) = ETAD(k+1) * (1.f - ptem * dz);
        }
    }
    pwevo = 0.f;                                                                      /* :1332-1347 */
    HCDO(jmin) = HEO(jmin); QCDO(jmin) = QO(jmin); QRCDO(jmin) = QESO(jmin);
    for (k = kmax1; k >= 1; k--)                                                      /* :1349-1372 */
        if (k < jmin) {
            dz = ZI(k+2) - ZI(k+1);
            if (k >= kbcon) { tem = xlamde * dz; tem1 = 0.5f * xlamdd * dz; }
            else { tem = xlamde * dz; tem1 = 0.5f * (xlamd + xlamdd) * dz; }
            factor = 1.f + tem - tem1;
            HCDO(k) = ((1.f - tem1) * HCDO(k+1) + tem * 0.5f * (HEO(k) + HEO(k+1))) / factor;
            DBYO(k) = HCDO(k) - HESO(k);
        }
    for (k = kmax1; k >= 1; k--)                                                      /* :1374-1398 */
        if (k < jmin) {
            dq = QESO(k);
            dt = TO(k);
            gamma = el2orc * dq / (dt * dt);
            QRCDO(k) = dq + (1.f / hvap_) * (gamma / (1.f + gamma)) * DBYO(k);
            dz = ZI(k+2) - ZI(k+1);
            if (k >= kbcon) { tem = xlamde * dz; tem1 = 0.5f * xlamdd * dz; }
            else { tem = xlamde * dz; tem1 = 0.5f * (xlamd + xlamdd) * dz; }
            factor = 1.f + tem - tem1;
            QCDO(k) = ((1.f - tem1) * QCDO(k+1) + tem * 0.5f * (QO(k) + QO(k+1))) / factor;
            PWDO(k) = ETAD(k+1) * QCDO(k) - ETAD(k+1) * QRCDO(k);
            QCDO(k) = QRCDO(k);
            pwevo = pwevo + PWDO(k);
        }
    edtmax = edtmaxl;                                                                 /* :1404-1415 */
    if (slimsk == 2.f) edtmax = edtmaxs;
    if (pwevo < 0.f) {
        edto = -edto * pwavo / pwevo;
        edto = NSAS_MIN(edto, edtmax);
    } else {
        edto = 0.f;
    }
    for (k = kmax1; k >= 1; k--)                                                      /* :1419-1437 */
        if (k < jmin) {
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            dhh = HCDO(k);
            dt = TO(k);
            dg = gamma;
            dh = HESO(k);
            dz = -1.f * (ZL(k+1) - ZL(k));
            aa1 = aa1 + edto * dz * (g_ / (cp_ * dt)) * ((dhh - dh) / (1.f + dg)) * (1.f + fv_ * cp_ * dg * dt / hvap_);
            aa1 = aa1 + edto * dz * g_ * fv_ * NSAS_MAX(0.f, (QESO(k) - QO(k)));
        }
    if (aa1 <= 0.f) return;
    if (edto > 0.f) NSAS_FLAG(NSAS_D_DOWNDRAFT);

    for (k = 1; k <= kmax; k++) { DELLAH(k) = 0.f; DELLAQ(k) = 0.f; }                 /* :1448-1471 */
    dp = 1000.f * DEL(1);
    DELLAH(1) = edto * ETAD(1) * (HCDO(1) - HEO(1)) * g_ / dp;
    DELLAQ(1) = edto * ETAD(1) * (QCDO(1) - QO(1)) * g_ / dp;
    for (k = 2; k <= kmax1; k++)                                                      /* :1475-1536 */
        if (k < ktcon) {
            aup = 1.f;
            if (k <= kb) aup = 0.f;
            adw = 1.f;
            if (k > jmin) adw = 0.f;
            dv1 = HEO(k);
            dv2 = .5f * (HEO(k) + HEO(k-1));
            dv3 = HEO(k-1);
            dv1q = QO(k);
            dv2q = .5f * (QO(k) + QO(k-1));
            dv3q = QO(k-1);
            dp = 1000.f * DEL(k);
            dz = ZI(k+1) - ZI(k);
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1));
            tem1 = xlamud;
            if (k <= kbcon) { ptem = xlamde; ptem1 = xlamd + xlamdd; }
            else { ptem = xlamde; ptem1 = xlamdd; }
            DELLAH(k) = DELLAH(k) +
                ((aup * ETA(k) - adw * edto * ETAD(k)) * dv1
                 - (aup * ETA(k-1) - adw * edto * ETAD(k-1)) * dv3
                 - (aup * tem * ETA(k-1) + adw * edto * ptem * ETAD(k)) * dv2 * dz
                 + aup * tem1 * ETA(k-1) * .5f * (HCKO(k) + HCKO(k-1)) * dz
                 + adw * edto * ptem1 * ETAD(k) * .5f * (HCDO(k) + HCDO(k-1)) * dz) * g_ / dp;
            DELLAQ(k) = DELLAQ(k) +
                ((aup * ETA(k) - adw * edto * ETAD(k)) * dv1q
                 - (aup * ETA(k-1) - adw * edto * ETAD(k-1)) * dv3q
                 - (aup * tem * ETA(k-1) + adw * edto * ptem * ETAD(k)) * dv2q * dz
                 + aup * tem1 * ETA(k-1) * .5f * (QCKO(k) + QCKO(k-1)) * dz
                 + adw * edto * ptem1 * ETAD(k) * .5f * (QRCDO(k) + QRCDO(k-1)) * dz) * g_ / dp;
        }
    indx = ktcon;                                                                     /* :1540-1561 */
    dp = 1000.f * DEL(indx);
    dv1 = HEO(indx-1);
    DELLAH(indx) = ETA(indx-1) * (HCKO(indx-1) - dv1) * g_ / dp;
    dvq1 = QO(indx-1);
    DELLAQ(indx) = ETA(indx-1) * (QCKO(indx-1) - dvq1) * g_ / dp;
    DELLAL(indx) = ETA(indx-1) * qlko_ktcon * g_ / dp;

    for (k = 1; k <= kmax; k++) {                                                     /* :1565-1578 */
        if (k > ktcon) { QO(k) = Q1(k); TO(k) = T1(k); }
        if (k <= ktcon) {
            QO(k) = DELLAQ(k) * mbdt + Q1(k);
            dellat = (DELLAH(k) - hvap_ * DELLAQ(k)) / cp_;
            TO(k) = dellat * mbdt + T1(k);
            QO(k) = NSAS_MAX(QO(k), 1.0e-10f);
        }
    }
    for (k = 1; k <= kmax; k++) QESO(k) = nsas_qes(TO(k), P(k), eps, qmin_, diag);    /* :1592-1601 */
    for (k = 1; k <= kmax1; k++) {                                                    /* :1612-1639 */
        dz = .5f * (ZL(k+1) - ZL(k));
        dp = .5f * (P(k+1) - P(k));
        es = 0.01f * nsas_fpvs(TO(k+1), diag);
        pprime = P(k+1) + (eps - 1.f) * es;
        qs = eps * es / pprime;
        dqsdp = -qs / pprime;
        desdt = es * (fact1 / TO(k+1) + fact2 / (TO(k+1) * TO(k+1)));
        dqsdt = qs * P(k+1) * desdt / (es * pprime);
        gamma = el2orc * QESO(k+1) / (TO(k+1) * TO(k+1));
        dt = (g_ * dz + hvap_ * dqsdp * dp) / (cp_ * (1.f + gamma));
        dq = dqsdt * dt + dqsdp * dp;
        TO(k) = TO(k+1) + dt;
        QO(k) = QO(k+1) + dq;
        po = .5f * (P(k) + P(k+1));
        QESO(k) = nsas_qes(TO(k), po, eps, qmin_, diag);
        QO(k) = NSAS_MAX(QO(k), 1.0e-10f);
        HEO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QO(k);
        HESO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QESO(k);
    }
    k = kmax;                                                                         /* :1641-1659 */
    HEO(k) = g_ * ZL(k) + cp_ * TO(k) + hvap_ * QO(k);
    HESO(k) = g_ * ZL(k) + cp_ * TO(k) + hvap_ * QESO(k);
    xaa0 = 0.f; xpwav = 0.f;
    HCKO(kb) = HEO(kb); QCKO(kb) = QO(kb);
    for (k = 2; k <= kmax1; k++)                                                      /* :1665-1676 */
        if (k > kb && k <= ktcon) {
            dz = ZI(k+1) - ZI(k);
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            HCKO(k) = ((1.f - tem1) * HCKO(k-1) + tem * 0.5f * (HEO(k) + HEO(k-1))) / factor;
        }
    for (k = 2; k <= kmax1; k++) {                                                    /* :1678-1721 */
        if (k > kb && k < ktcon) {
            dz = ZI(k+1) - ZI(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            xdby = HCKO(k) - HESO(k);
            xqrch = QESO(k) + gamma * xdby / (hvap_ * (1.f + gamma));
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            QCKO(k) = ((1.f - tem1) * QCKO(k-1) + tem * 0.5f * (QO(k) + QO(k-1))) / factor;
            dq = ETA(k) * QCKO(k) - ETA(k) * xqrch;
            if (k >= kbcon && dq > 0.f) {
                etah = .5f * (ETA(k) + ETA(k-1));
                if (k > jmin) qlk = dq / (ETA(k) + etah * (c0 + c1) * dz);
                else qlk = dq / (ETA(k) + etah * c0 * dz);
                if (k < ktcon1) xaa0 = xaa0 - dz * g_ * qlk;
                QCKO(k) = qlk + xqrch;
                xpw = etah * c0 * dz * qlk;
                xpwav = xpwav + xpw;
            }
        }
        if (k >= kbcon && k < ktcon1) {
            dz1 = ZL(k+1) - ZL(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            rfact = 1.f + fv_ * cp_ * gamma * TO(k) / hvap_;
            xdby = HCKO(k) - HESO(k);
            xaa0 = xaa0 + dz1 * (g_ / (cp_ * TO(k))) * xdby / (1.f + gamma) * rfact;
            xaa0 = xaa0 + dz1 * g_ * fv_ * NSAS_MAX(0.f, (QESO(k) - QO(k)));
        }
    }
    xpwev = 0.f;                                                                      /* :1728-1739 */
    XHCD(jmin) = HEO(jmin); XQCD(jmin) = QO(jmin);
    for (k = kmax1; k >= 1; k--)                                                      /* :1741-1757 */
        if (k < jmin) {
            dz = ZI(k+2) - ZI(k+1);
            if (k >= kbcon) { tem = xlamde * dz; tem1 = 0.5f * xlamdd * dz; }
            else { tem = xlamde * dz; tem1 = 0.5f * (xlamd + xlamdd) * dz; }
            factor = 1.f + tem - tem1;
            XHCD(k) = ((1.f - tem1) * XHCD(k+1) + tem * 0.5f * (HEO(k) + HEO(k+1))) / factor;
        }
    for (k = kmax1; k >= 1; k--)                                                      /* :1759-1783 */
        if (k < jmin) {
            dq = QESO(k);
            dt = TO(k);
            gamma = el2orc * dq / (dt * dt);
            dh = XHCD(k) - HESO(k);
            qrcd = dq + (1.f / hvap_) * (gamma / (1.f + gamma)) * dh;
            dz = ZI(k+2) - ZI(k+1);
            if (k >= kbcon) { tem = xlamde * dz; tem1 = 0.5f * xlamdd * dz; }
            else { tem = xlamde * dz; tem1 = 0.5f * (xlamd + xlamdd) * dz; }
            factor = 1.f + tem - tem1;
            XQCD(k) = ((1.f - tem1) * XQCD(k+1) + tem * 0.5f * (QO(k) + QO(k+1))) / factor;
            xpwd = ETAD(k+1) * (XQCD(k) - qrcd);
            XQCD(k) = qrcd;
            xpwev = xpwev + xpwd;
        }
    edtmax = edtmaxl;                                                                 /* :1785-1796 */
    if (slimsk == 2.f) edtmax = edtmaxs;
    if (xpwev >= 0.f) {
        edtx = 0.f;
    } else {
        edtx = -edtx * xpwav / xpwev;
        edtx = NSAS_MIN(edtx, edtmax);
    }
    for (k = kmax1; k >= 1; k--)                                                      /* :1800-1815 */
        if (k < jmin) {
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            dhh = XHCD(k);
            dt = TO(k);
            dg = gamma;
            dh = HESO(k);
            dz = -1.f * (ZL(k+1) - ZL(k));
            xaa0 = xaa0 + edtx * dz * (g_ / (cp_ * dt)) * ((dhh - dh) / (1.f + dg)) * (1.f + fv_ * cp_ * dg * dt / hvap_);
            xaa0 = xaa0 + edtx * dz * g_ * fv_ * NSAS_MAX(0.f, (QESO(k) - QO(k)));
        }
    if (P(ktcon) < pcrit[14]) {                                                       /* :1819-1834, acrit(k) of :612-614 made in place */
        acrt = (acritt[14] * (975.f - pcrit[14])) * (975.f - P(ktcon)) / (975.f - pcrit[14]);
    } else if (P(ktcon) > pcrit[0]) {
        acrt = acritt[0] * (975.f - pcrit[0]);
    } else {
        k = (int)((850.f - P(ktcon)) / 50.f) + 2;
        k = NSAS_MIN(k, 15);
        k = NSAS_MAX(k, 2);
        const float ak = acritt[k-1] * (975.f - pcrit[k-1]), akm = acritt[k-2] * (975.f - pcrit[k-2]);
        acrt = ak + (akm - ak) * (P(ktcon) - pcrit[k-1]) / (pcrit[k-2] - pcrit[k-1]);
    }
    w1 = W1s; w2 = W2s; w3 = W3s; w4 = W4s;                                           /* :1836-1864 */
    if (slimsk == 1.f) { w1 = W1l; w2 = W2l; w3 = W3l; w4 = W4l; }
    if (pdot <= w4) acrtfct = (pdot - w4) / (w3 - w4);
    else if (pdot >= -w4) acrtfct = -(pdot + w4) / (w4 - w3);
    else acrtfct = 0.f;
    acrtfct = NSAS_MAX(acrtfct, -1.f);
    acrtfct = NSAS_MIN(acrtfct, 1.f);
    acrtfct = 1.f - acrtfct;
    dtconv = dt2 + NSAS_MAX((1800.f - dt2), 0.f) * (pdot - w2) / (w1 - w2);
    dtconv = NSAS_MAX(dtconv, dtmin);
    dtconv = NSAS_MIN(dtconv, dtmax);
    f = (aa1 - acrt * acrtfct) / dtconv;                                              /* :1868-1893 */
    if (f <= 0.f) return;
    xk = (xaa0 - aa1) / mbdt;
    if (xk >= 0.f) return;
    xmb = -f / xk;
    xmb = NSAS_MIN(xmb, xmbmax);

    NSAS_FLAG(NSAS_D_DEEP_END);
    for (k = 1; k <= kmax; k++) {                                                     /* :1897-1909 */
        TO(k) = T1(k);
        QO(k) = Q1(k);
        QESO(k) = nsas_qes(T1(k), P(k), eps, qmin_, diag);
    }
    for (k = 1; k <= kmax; k++)                                                       /* :1925-1946 */
        if (k <= ktcon) {
            dellat = (DELLAH(k) - hvap_ * DELLAQ(k)) / cp_;
            T1(k) = T1(k) + dellat * xmb * dt2;
            Q1(k) = Q1(k) + DELLAQ(k) * xmb * dt2;
        }
    for (k = 1; k <= kmax; k++)                                                       /* :1953-1961 */
        if (k <= ktcon) QESO(k) = nsas_qes(T1(k), P(k), eps, qmin_, diag);
    rntot = 0.f; delqev = 0.f; delq2 = 0.f; flg = 1; qcond = 0.f;                     /* :1963-1984 */
    for (k = kmax; k >= 1; k--)
        if (k < ktcon) {
            aup = 1.f;
            if (k <= kb) aup = 0.f;
            adw = 1.f;
            if (k >= jmin) adw = 0.f;
            rntot = rntot + (aup * PWO(k) + adw * edto * PWDO(k)) * xmb * .001f * dt2;
        }
    for (k = kmax; k >= 1; k--) {                                                     /* :1988-2031 */
        qevap = 0.0f;
        if (k < ktcon) {
            aup = 1.f;
            if (k <= kb) aup = 0.f;
            adw = 1.f;
            if (k >= jmin) adw = 0.f;
            rain = rain + (aup * PWO(k) + adw * edto * PWDO(k)) * xmb * .001f * dt2;
        }
        if (flg && k < ktcon) {
            evef = edt * evfacts;
            if (slimsk == 1.f) evef = edt * evfactl;
            qcond = evef * (Q1(k) - QESO(k)) / (1.f + el2orc * QESO(k) / (T1(k) * T1(k)));
            dp = 1000.f * DEL(k);
            if (rain > 0.f && qcond < 0.f) {
                qevap = -qcond * (1.f - NSAS_EXPF(-.32f * NSAS_SQRTF(dt2 * rain)));
                qevap = NSAS_MIN(qevap, rain * 1000.f * g_ / dp);
                delq2 = delqev + .001f * qevap * dp / g_;
                if (delq2 > rntot) {
                    qevap = 1000.f * g_ * (rntot - delqev) / dp;
                    flg = 0;
                    NSAS_FLAG(NSAS_D_EVAP_CUT);
                }
            }
            if (rain > 0.f && qevap > 0.f) {
                Q1(k) = Q1(k) + qevap;
                T1(k) = T1(k) - (hvap_ / cp_) * qevap;
                rain = rain - .001f * qevap * dp / g_;
                delqev = delqev + .001f * dp * qevap / g_;
                NSAS_FLAG(NSAS_D_EVAP);
            }
        }
    }
    if (rain < 0.f && !flg) rain = 0.f;                                               /* :2036-2047 */
    if (rain <= 0.f) {
        rain = 0.f;
    } else {
        o->ktop = ktcon;
        o->kbot = kbcon;
        o->icps = 1;
        NSAS_FLAG(NSAS_D_DEEP_RAIN);
    }
    o->rain1 = rain;
    if (rain <= 0.f) {                                                                /* :2049-2058 */
        for (k = 1; k <= kmax; k++) { T1(k) = TO(k); Q1(k) = QO(k); }
        NSAS_FLAG(NSAS_D_RESTORED);
    }
    if (rain > 0.f)                                                                   /* :2062-2079 */
        for (k = 1; k <= kmax; k++)
            if (k >= kbcon && k <= ktcon) {
                tem = DELLAL(k) * xmb * dt2;
                tem1 = NSAS_MAX(0.0f, NSAS_MIN(1.0f, (tcr - T1(k)) * tcrf));
                QI2(k) = QI2(k) + tem * tem1;
                QC2(k) = QC2(k) + tem * (1.0f - tem1);
                if (tem > 0.f) NSAS_FLAG(tem1 == 1.0f ? NSAS_D_ICE_ONLY : tem1 == 0.0f ? NSAS_D_WATER_ONLY : NSAS_D_MIXED);
            }
}

/* nscv2d :2339-3288 for one column, after nsas_deep on the same workspace */
NSAS_FN void nsas_shallow(NsasIn in, int n, float slimsk, float hpbl, float hfx, float qfx, float delt, float *ws, size_t stride,
                          size_t nl, NsasOut *o, int *diag)
{
    const float c0 = .002f, c1 = 5.e-4f, cincrmax = 180.f, cincrmin = 120.f, dthk = 25.f, h1 = 0.33333333f;
    const float tf = 233.16f, tcr = 263.16f, tcrf = 1.0f / (tcr - tf);
    const float g_ = NSAS_G, cp_ = NSAS_CP, hvap_ = NSAS_HVAP, rv_ = NSAS_RV, rd_ = NSAS_RD, fv_ = NSAS_FV, pgcon = NSAS_PGCON;
    const float t0c_ = NSAS_T0C;
    const int km1 = n - 1;
    float dz, dp, es, pprime, qs, dqsdp, desdt, dqsdt, gamma, dt, dq, tem, tem1, factor, ptem, ptem1, dz1, qrch, etah, qlk, rfact, shear,
          e1, dellat, evef, cincr, dv1h, dv2h, dv3h, dv1q, dv2q, dv3q, val, val1, val2;
    float hmax, pdot, xlamud, aa1, xmbmax, qlko_ktcon, vshear, edt, xmb, rntot, delqev, delq2, qcond, qevap, rain, wstar;
    int kb, kbcon, kbcon1, ktcon, ktcon1, kbm, kmax, kpbl, flg, k, indx, kk;
    (void)pgcon;

    const float thx1 = T1(1) / in.pi[0];                                              /* :2347-2361 */
    const float tvcon = (1.f + fv_ * Q1(1));
    const float rhox = PRSL(1) * 1.e3f / (rd_ * T1(1) * tvcon);
    const float sflx = hfx / rhox / cp_ + qfx / rhox * fv_ * thx1;
    o->rain2 = 0.f;                                                                   /* :2365-2382 */
    if (sflx <= 0.f) NSAS_FLAG(NSAS_D_SFLX_NEG);
    if (o->icps == 1 || sflx <= 0.f) return;
    o->kbot = n + 1; o->ktop = 0;
    rain = 0.f; qlko_ktcon = 0.f; edt = 0.f; aa1 = 0.f; vshear = 0.f;

    const float dt2 = delt;                                                           /* :2390-2419 */
    const float clam = .3f, aafac = .1f, betaw = .03f, evfact = 0.3f, evfactl = 0.3f;
    const float el2orc = hvap_ * hvap_ / (rv_ * cp_);
    const float eps = rd_ / rv_;
    const float fact1 = (NSAS_CVAP - NSAS_CLIQ) / rv_;
    const float fact2 = hvap_ / rv_ - fact1 * t0c_;
    const float w1l = -8.e-3f, w2l = -4.e-2f, w3l = -5.e-3f, w4l = -5.e-4f, w1s = -2.e-4f, w2s = -2.e-3f, w3s = -1.e-3f, w4s = -2.e-5f;
    float w3, w4;
    (void)w1l; (void)w2l; (void)w1s; (void)w2s;

    kbm = n; kmax = n;                                                                /* :2424-2438 */
    for (k = 1; k <= n; k++) {
        if (PRSL(k) > in.pint[0] * 0.001f * 0.70f) kbm = k + 1;
        if (PRSL(k) > in.pint[0] * 0.001f * 0.60f) kmax = k + 1;
    }
    kbm = NSAS_MIN(kbm, kmax);
    for (k = 2; k <= n; k++) ZI(k) = 0.5f * (ZL(k-1) + ZL(k));                        /* :2443-2457 */
    for (k = 1; k <= km1; k++) XLAMB(k) = clam / ZI(k+1);
    XLAMB(n) = XLAMB(km1);
    flg = 1; kpbl = 1;                                                                /* :2461-2478 */
    for (k = 2; k <= km1; k++) {
        if (flg && ZL(k) <= hpbl) kpbl = k;
        else flg = 0;
    }
    kpbl = NSAS_MIN(kpbl, kbm);
    for (k = 1; k <= n; k++)                                                          /* :2483-2501 */
        if (k <= kmax) {
            P(k) = PRSL(k) * 10.0f;
            ETA(k) = 1.f; HCKO(k) = 0.f; QCKO(k) = 0.f; DBYO(k) = 0.f; PWO(k) = 0.f; DELLAL(k) = 0.f;
            TO(k) = T1(k); QO(k) = Q1(k);
            UO(k) = in.u[(size_t)(k - 1) * in.ls]; VO(k) = in.v[(size_t)(k - 1) * in.ls];
        }
    for (k = 1; k <= n; k++)                                                          /* :2511-2534 */
        if (k <= kmax) {
            val1 = 1.e-8f;
            QESO(k) = nsas_qes(TO(k), P(k), eps, val1, diag);
            val2 = 1.e-10f;
            QO(k) = NSAS_MAX(QO(k), val2);
            tem = g_ * ZL(k) + cp_ * TO(k);
            HEO(k) = tem + hvap_ * QO(k);
            HESO(k) = tem + hvap_ * QESO(k);
        }
    hmax = HEO(1); kb = 1;                                                            /* :2539-2555 */
    for (k = 2; k <= n; k++)
        if (k <= kpbl) {
            if (HEO(k) > hmax) { kb = k; hmax = HEO(k); }
        }
    for (k = 1; k <= km1; k++)                                                        /* :2557-2576 */
        if (k <= kmax - 1) {
            dz = .5f * (ZL(k+1) - ZL(k));
            dp = .5f * (P(k+1) - P(k));
            es = 0.01f * nsas_fpvs(TO(k+1), diag);
            pprime = P(k+1) + (eps - 1.f) * es;
            qs = eps * es / pprime;
            dqsdp = -qs / pprime;
            desdt = es * (fact1 / TO(k+1) + fact2 / (TO(k+1) * TO(k+1)));
            dqsdt = qs * P(k+1) * desdt / (es * pprime);
            gamma = el2orc * QESO(k+1) / (TO(k+1) * TO(k+1));
            dt = (g_ * dz + hvap_ * dqsdp * dp) / (cp_ * (1.f + gamma));
            dq = dqsdt * dt + dqsdp * dp;
            TO(k) = TO(k+1) + dt;
            QO(k) = QO(k+1) + dq;
            PO(k) = .5f * (P(k) + P(k+1));
        }
    for (k = 1; k <= km1; k++)                                                        /* :2578-2595 */
        if (k <= kmax - 1) {
            val1 = 1.e-8f;
            QESO(k) = nsas_qes(TO(k), PO(k), eps, val1, diag);
            val2 = 1.e-10f;
            QO(k) = NSAS_MAX(QO(k), val2);
            HEO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QO(k);
            HESO(k) = .5f * g_ * (ZL(k) + ZL(k+1)) + cp_ * TO(k) + hvap_ * QESO(k);
            UO(k) = .5f * (UO(k) + UO(k+1));
            VO(k) = .5f * (VO(k) + VO(k+1));
        }
    flg = 1; kbcon = kmax;                                                            /* :2599-2619 */
    for (k = 2; k <= km1; k++)
        if (flg && k < kbm) {
            if (k > kb && HEO(kb) > HESO(k)) { kbcon = k; flg = 0; }
        }
    if (kbcon == kmax) return;

    pdot = 10.f * nsas_dot(in, kbcon);                                                /* :2630-2668 */
    if (slimsk == 1.f) { w3 = w3l; w4 = w4l; } else { w3 = w3s; w4 = w4s; }
    if (pdot <= w4) ptem = (pdot - w4) / (w3 - w4);
    else if (pdot >= -w4) ptem = -(pdot + w4) / (w4 - w3);
    else ptem = 0.f;
    val1 = -1.f;
    ptem = NSAS_MAX(ptem, val1);
    val2 = 1.f;
    ptem = NSAS_MIN(ptem, val2);
    ptem = 1.f - ptem;
    ptem1 = .5f * (cincrmax - cincrmin);
    cincr = cincrmax - ptem * ptem1;
    tem1 = P(kb) - P(kbcon);
    if (tem1 > cincr) return;

    xlamud = XLAMB(kbcon);                                                            /* :2679-2683 */
    for (k = km1; k >= 1; k--)                                                        /* :2687-2697 */
        if (k < kbcon && k >= kb) {
            dz = ZI(k+2) - ZI(k+1);
            ptem = 0.5f * (XLAMB(k) + XLAMB(k+1)) - xlamud;
            ETA(k) = ETA(k+1) / (1.f + ptem * dz);
        }
    for (k = 2; k <= km1; k++)                                                        /* :2701-2711 */
        if (k > kbcon && k < kmax) {
            dz = ZI(k+1) - ZI(k);
            ptem = 0.5f * (XLAMB(k) + XLAMB(k-1)) - xlamud;
            ETA(k) = ETA(k-1) * (1.f + ptem * dz);
        }
    HCKO(kb) = HEO(kb);                                                               /* :2715-2744 */
    for (k = 2; k <= km1; k++)
        if (k > kb && k < kmax) {
            dz = ZI(k+1) - ZI(k);
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            HCKO(k) = ((1.f - tem1) * HCKO(k-1) + tem * 0.5f * (HEO(k) + HEO(k-1))) / factor;
            DBYO(k) = HCKO(k) - HESO(k);
        }
    flg = 1; kbcon1 = kmax;                                                           /* :2749-2778 */
    for (k = 2; k <= km1; k++)
        if (flg && k < kbm) {
            if (k >= kbcon && DBYO(k) > 0.f) { kbcon1 = k; flg = 0; }
        }
    if (kbcon1 == kmax) return;
    tem = P(kbcon) - P(kbcon1);
    if (tem > dthk) return;

    flg = 1; ktcon = kbm;                                                             /* :2789-2803 */
    for (k = 2; k <= km1; k++)
        if (flg && k < kbm) {
            if (k > kbcon1 && DBYO(k) < 0.f) { ktcon = k; flg = 0; }
        }
    dp = 1000.f * DEL(kbcon);                                                         /* :2807-2813 */
    xmbmax = dp / (g_ * dt2);
    aa1 = 0.f;                                                                        /* :2817-2858 */
    QCKO(kb) = QO(kb);
    for (k = 2; k <= km1; k++)
        if (k > kb && k < ktcon) {
            dz = ZI(k+1) - ZI(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            QCKO(k) = ((1.f - tem1) * QCKO(k-1) + tem * 0.5f * (QO(k) + QO(k-1))) / factor;
            dq = ETA(k) * (QCKO(k) - qrch);
            if (k >= kbcon && dq > 0.f) {
                etah = .5f * (ETA(k) + ETA(k-1));
                dp = 1000.f * DEL(k);
                qlk = dq / (ETA(k) + etah * (c0 + c1) * dz);
                DELLAL(k) = etah * c1 * dz * qlk * g_ / dp;
                aa1 = aa1 - dz * g_ * qlk;
                QCKO(k) = qlk + qrch;
                PWO(k) = etah * c0 * dz * qlk;
            }
        }
    for (k = 2; k <= km1; k++)                                                        /* :2862-2880 */
        if (k >= kbcon && k < ktcon) {
            dz1 = ZL(k+1) - ZL(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            rfact = 1.f + fv_ * cp_ * gamma * TO(k) / hvap_;
            aa1 = aa1 + dz1 * (g_ / (cp_ * TO(k))) * DBYO(k) / (1.f + gamma) * rfact;
            val = 0.f;
            aa1 = aa1 + dz1 * g_ * fv_ * NSAS_MAX(val, (QESO(k) - QO(k)));
        }
    if (aa1 <= 0.f) return;

    aa1 = aafac * aa1;                                                                /* :2892-2921 */
    flg = 1; ktcon1 = kbm;
    for (k = 2; k <= km1; k++)
        if (flg) {
            if (k >= ktcon && k < kbm) {
                dz1 = ZL(k+1) - ZL(k);
                gamma = el2orc * QESO(k) / (TO(k) * TO(k));
                rfact = 1.f + fv_ * cp_ * gamma * TO(k) / hvap_;
                aa1 = aa1 + dz1 * (g_ / (cp_ * TO(k))) * DBYO(k) / (1.f + gamma) * rfact;
                if (aa1 < 0.f) { ktcon1 = k; flg = 0; }
            }
        }
    for (k = 2; k <= km1; k++)                                                        /* :2926-2958 */
        if (k >= ktcon && k < ktcon1) {
            dz = ZI(k+1) - ZI(k);
            gamma = el2orc * QESO(k) / (TO(k) * TO(k));
            qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1)) * dz;
            tem1 = 0.5f * xlamud * dz;
            factor = 1.f + tem - tem1;
            QCKO(k) = ((1.f - tem1) * QCKO(k-1) + tem * 0.5f * (QO(k) + QO(k-1))) / factor;
            dq = ETA(k) * (QCKO(k) - qrch);
            if (dq > 0.f) {
                etah = .5f * (ETA(k) + ETA(k-1));
                dp = 1000.f * DEL(k);
                qlk = dq / (ETA(k) + etah * (c0 + c1) * dz);
                DELLAL(k) = etah * c1 * dz * qlk * g_ / dp;
                QCKO(k) = qlk + qrch;
                PWO(k) = etah * c0 * dz * qlk;
            }
        }
    kk = ktcon; ktcon = ktcon1; ktcon1 = kk;                                          /* :2962-2968 */
    k = ktcon - 1;                                                                    /* :2976-2991 */
    gamma = el2orc * QESO(k) / (TO(k) * TO(k));
    qrch = QESO(k) + gamma * DBYO(k) / (hvap_ * (1.f + gamma));
    dq = QCKO(k) - qrch;
    if (dq > 0.f) { qlko_ktcon = dq; QCKO(k) = qrch; }

    vshear = 0.f;                                                                     /* :2997-3025 */
    for (k = 2; k <= n; k++)
        if (k > kb && k <= ktcon) {
            shear = NSAS_SQRTF((UO(k) - UO(k-1)) * (UO(k) - UO(k-1)) + (VO(k) - VO(k-1)) * (VO(k) - VO(k-1)));
            vshear = vshear + shear;
        }
    vshear = 1.e3f * vshear / (ZI(ktcon+1) - ZI(kb+1));
    e1 = 1.591f - .639f * vshear + .0953f * (vshear * vshear) - .00496f * (vshear * vshear * vshear);
    edt = 1.f - e1;
    val = .9f;
    edt = NSAS_MIN(edt, val);
    val = .0f;
    edt = NSAS_MAX(edt, val);

    for (k = 1; k <= n; k++)                                                          /* :3030-3039 */
        if (k <= kmax) { DELLAH(k) = 0.f; DELLAQ(k) = 0.f; }
    for (k = 2; k <= km1; k++)                                                        /* :3043-3091 */
        if (k > kb && k < ktcon) {
            dp = 1000.f * DEL(k);
            dz = ZI(k+1) - ZI(k);
            dv1h = HEO(k);
            dv2h = .5f * (HEO(k) + HEO(k-1));
            dv3h = HEO(k-1);
            dv1q = QO(k);
            dv2q = .5f * (QO(k) + QO(k-1));
            dv3q = QO(k-1);
            tem = 0.5f * (XLAMB(k) + XLAMB(k-1));
            tem1 = xlamud;
            DELLAH(k) = DELLAH(k) +
                (ETA(k) * dv1h - ETA(k-1) * dv3h
                 - tem * ETA(k-1) * dv2h * dz
                 + tem1 * ETA(k-1) * .5f * (HCKO(k) + HCKO(k-1)) * dz) * g_ / dp;
            DELLAQ(k) = DELLAQ(k) +
                (ETA(k) * dv1q - ETA(k-1) * dv3q
                 - tem * ETA(k-1) * dv2q * dz
                 + tem1 * ETA(k-1) * .5f * (QCKO(k) + QCKO(k-1)) * dz) * g_ / dp;
        }
    indx = ktcon;                                                                     /* :3095-3117 */
    dp = 1000.f * DEL(indx);
    dv1h = HEO(indx-1);
    DELLAH(indx) = ETA(indx-1) * (HCKO(indx-1) - dv1h) * g_ / dp;
    dv1q = QO(indx-1);
    DELLAQ(indx) = ETA(indx-1) * (QCKO(indx-1) - dv1q) * g_ / dp;
    DELLAL(indx) = ETA(indx-1) * qlko_ktcon * g_ / dp;

    k = kbcon;                                                                        /* :3122-3131 */
    ptem = g_ * sflx * hpbl / T1(1);
    wstar = NSAS_POWF(ptem, h1);
    tem = PO(k) * 100.f / (rd_ * T1(k));
    xmb = betaw * tem * wstar;
    xmb = NSAS_MIN(xmb, xmbmax);
    for (k = 1; k <= n; k++)                                                          /* :3133-3142 */
        if (k <= kmax) QESO(k) = nsas_qes(T1(k), P(k), eps, 1.e-8f, diag);
    qcond = 0.f;
    for (k = 1; k <= n; k++)                                                          /* :3153-3172 */
        if (k > kb && k <= ktcon) {
            dellat = (DELLAH(k) - hvap_ * DELLAQ(k)) / cp_;
            T1(k) = T1(k) + dellat * xmb * dt2;
            Q1(k) = Q1(k) + DELLAQ(k) * xmb * dt2;
        }
    for (k = 1; k <= n; k++)                                                          /* :3174-3186 */
        if (k > kb && k <= ktcon) QESO(k) = nsas_qes(T1(k), P(k), eps, 1.e-8f, diag);
    rntot = 0.f; delqev = 0.f; delq2 = 0.f; flg = 1;                                  /* :3188-3203 */
    for (k = n; k >= 1; k--)
        if (k < ktcon && k > kb) rntot = rntot + PWO(k) * xmb * .001f * dt2;
    for (k = n; k >= 1; k--)                                                          /* :3207-3254 */
        if (k <= kmax) {
            qevap = 0.f;
            if (k < ktcon && k > kb) rain = rain + PWO(k) * xmb * .001f * dt2;
            if (flg && k < ktcon) {
                evef = edt * evfact;
                if (slimsk == 1.f) evef = edt * evfactl;
                qcond = evef * (Q1(k) - QESO(k)) / (1.f + el2orc * QESO(k) / (T1(k) * T1(k)));
                dp = 1000.f * DEL(k);
                if (rain > 0.f && qcond < 0.f) {
                    qevap = -qcond * (1.f - NSAS_EXPF(-.32f * NSAS_SQRTF(dt2 * rain)));
                    qevap = NSAS_MIN(qevap, rain * 1000.f * g_ / dp);
                    delq2 = delqev + .001f * qevap * dp / g_;
                }
                if (rain > 0.f && qcond < 0.f && delq2 > rntot) {
                    qevap = 1000.f * g_ * (rntot - delqev) / dp;
                    flg = 0;
                }
                if (rain > 0.f && qevap > 0.f) {
                    tem = .001f * dp / g_;
                    tem1 = qevap * tem;
                    if (tem1 > rain) {
                        qevap = rain / tem;
                        rain = 0.f;
                    } else {
                        rain = rain - tem1;
                    }
                    Q1(k) = Q1(k) + qevap;
                    T1(k) = T1(k) - (hvap_ / cp_) * qevap;
                    delqev = delqev + .001f * dp * qevap / g_;
                    NSAS_FLAG(NSAS_D_SHALLOW_EVAP);
                }
            }
        }
    if (rain < 0.f || !flg) rain = 0.f;                                               /* :3256-3263 */
    o->rain2 = rain;
    o->ktop = ktcon;
    o->kbot = kbcon;
    o->icps = 0;
    NSAS_FLAG(NSAS_D_SHALLOW);
    for (k = 1; k <= km1; k++)                                                        /* :3269-3284 */
        if (k >= kbcon && k <= ktcon) {
            tem = DELLAL(k) * xmb * dt2;
            tem1 = NSAS_MAX(0.0f, NSAS_MIN(1.0f, (tcr - T1(k)) * tcrf));
            QI2(k) = QI2(k) + tem * tem1;
            QC2(k) = QC2(k) + tem * (1.0f - tem1);
            if (tem > 0.f) NSAS_FLAG(tem1 == 1.0f ? NSAS_D_ICE_ONLY : tem1 == 0.0f ? NSAS_D_WATER_ONLY : NSAS_D_MIXED);
        }
}

/* cu_nsas :231-303 for one column: the two rains (STEPCU = 1) and the four tendencies; element k of a result at [k * ls] */
NSAS_FN void nsas_finish(NsasIn in, int n, float dt, const float *ws, size_t stride, size_t nl, const NsasOut *o, float *tend_th,
                         float *tend_qv, float *tend_qc, float *tend_qi, float *raincv, float *pratec, float *hbot, float *htop)
{
    const float delt = dt * 1.f, rdelt = 1.f / delt;
    const float pratec1 = o->rain1 * 1000.f / (1.f * dt), raincv1 = o->rain1 * 1000.f / 1.f;
    const float pratec2 = o->rain2 * 1000.f / (1.f * dt), raincv2 = o->rain2 * 1000.f / 1.f;
    *raincv = raincv1 + raincv2;
    *pratec = pratec1 + pratec2;
    *hbot = (float)o->kbot;
    *htop = (float)o->ktop;
    for (int k = 1; k <= n; k++) {
        const size_t a = (size_t)(k - 1) * in.ls;
        tend_th[a] = (T1(k) - in.t[a]) / in.pi[a] * rdelt;
        tend_qv[a] = (Q1(k) - in.qv[a]) * rdelt;
        tend_qi[a] = (QI2(k) - in.qi[a]) * rdelt;
        tend_qc[a] = (QC2(k) - in.qc[a]) * rdelt;
    }
}

#undef DEL
#undef ZL
#undef PRSL
#undef T1
#undef Q1
#undef QC2
#undef QI2
#undef P
#undef TO
#undef QO
#undef UO
#undef VO
#undef QESO
#undef HEO
#undef HESO
#undef DBYO
#undef FRH
#undef FENT1
#undef FENT2
#undef XLAMB
#undef ETA
#undef ETAD
#undef HCKO
#undef QCKO
#undef HCDO
#undef QCDO
#undef QRCDO
#undef PWO
#undef PWDO
#undef DELLAL
#undef DELLAH
#undef DELLAQ
#undef XHCD
#undef XQCD
#undef ZI
#undef PO

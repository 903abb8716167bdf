// icar_amd/csrc/tiedtke_column.h -- one column of the Tiedtke convection scheme as cu_driver.f90 calls it (convection = kCU_TIEDTKE),
// for the device (cu_tiedtke.hip) and for the host (tests/support/tiedtke_oracle.c compiles this very file with a C compiler).
//
// Reference algorithm: src/physics/cu_tiedtke.f90 -- the per-row body of CU_TIEDTKE :362-488, TIECNV :573-711, CUMASTR_NEW :721-1244,
// CUINI :1256-1388, CUBASE :1393-1537, CUASC_NEW :1882-2382, CUDLFS :2388-2524, CUDDRAF :2530-2666, CUFLX :2672-2840, CUDTDQ
// :2846-2968, CUBASMC :3087-3164, CUADJTQ :3170-3325, CUENTR_NEW :3331-3443, TLUCUA / TLUCUB / TLUCUC :3470-3527, with the arguments
// of src/physics/cu_driver.f90:303-330 (itimestep = STEPCU = 1, levels kts .. kte-1).  REAL(4) in the reference's operation order, no
// contraction, IEEE division and square root; every PARAMETER expression is written as the reference writes it so that it folds in
// REAL(4).  exp is the C library's (the includer names it: TDK_EXPF; TDK_SQRTF likewise).  Every ** that is evaluated is an integer
// power and a product in the compiled reference.
//
// What cu_driver's arguments leave of the scheme.  itimestep = 1 makes Q1B = Q1BL = 0 (:406-408), so PQTE = +0 on entry.  Then
//   ZDQCV = sum 0 * dp = 0 and `ZDQCV > MAX(0., 1.1*PQHFL*G)` is false for every PQHFL: KTYPE = 2 at :905-909, never 1;
//   ZDQPBL = 0, so :931 takes its ELSE: ZMFUB = 0.01, LDCUM = .FALSE. for every column before the first ascent;
//   CUASC_NEW sets KTYPE = 0 where LDCUM is false (:2016), and the only statement that sets it afterwards is CUBASMC's KTYPE = 3.
// KTYPE is therefore 0 or 3 from :2016 on.  Not built because never evaluated: every `KTYPE .EQ. 1` and `KTYPE .EQ. 2` branch
// (:980-1009 IHMIN, :1036-1040, :1087-1136 the CAPE closure with its KTOP0, :2056-2086, :2182-2192, :2302-2330, CUENTR_NEW's
// organized detrainment with TAN :3422-3439, LLO1 of :1160), ZHHATT (read only there), ZOENTR / ZODETR as arrays (they stay +0; the
// statements that read them are kept, with the zeros as scalars), the surface fluxes QFX / HFX and rho2d (read by the KTYPE test
// above and by CUTYPE only), CUTYPE (cutrigger = 1), the orgen = 2 / nturben = 2 branches, CUDUDV and every momentum array (the
// winds are passive: cu_driver.f90:502-507 is commented out), PSRAIN / PSEVAP / PSHEAT / PSDISS / PSMELT, PAPRC / PAPRS.
// tests/golden/make_golden_tiedtke.py refuses to write vectors unless this very code reproduces the compiled reference bit for bit.
//
// Values shared along a row of the reference.  The early exits (ICUM :1029, IS .EQ. 0 :1483 :2143 :2352 :2478 :2597, ISUM .EQ. 0 in
// CUADJTQ, ITOPM2) guard work that is also guarded per column or acts on zeros; CUADJTQ's second iteration with KCALL = 0 is always
// run here (for a column with ZCOND = 0 it recomputes the same zero).  `leveltop` (:2098-2106) IS a row dependence: it is made from
// the pressure of the row's first column and is an argument of tdk_column (tdk_leveltop makes it).
//
// The level arrays of a column live in a workspace laid out [array][level][column]: TDK_WS(a, k) is level k (1-based, 1 = top: the
// scheme's flipped order) of array a; `stride` is the number of columns the workspace holds (1 on the host), `nl` its level count
// (>= n + 1).  Arrays of the reference that are not stored: PTEN / PAP / PAPH (read from the model's arrays through the flip),
// PTTE / PQTE / PCTE / ZQQ (made and consumed level by level), ZTENWB / ZQENWB / ZQOLD (read only at the level that made them),
// ZOENTR / ZODETR / ZHHATT and the eight momentum arrays (see above).
//
// Levels: n = kte - 1 scheme levels.  n >= TDK_MIN_LEVELS: with n = 2 KCBOT = KLEVM1 = 1 and :937 reads PAPH(JL,IKB-1) = PAPH(JL,0)
// above the column (tests/support/tiedtke_bounds_main.c finds the count).
#pragma once
#include <stddef.h>

#ifndef TDK_FN
#define TDK_FN static inline
#endif

enum { TDK_PQEN = 0, TDK_PQSEN, TDK_PGEO, TDK_PVERV, TDK_GEOH, TDK_TENH, TDK_QENH, TDK_QSENH, TDK_PTU, TDK_PQU, TDK_PLU, TDK_PLUDE, TDK_PMFU,
       TDK_PMFD, TDK_MFUS, TDK_MFDS, TDK_MFUQ, TDK_MFDQ, TDK_DMFUP, TDK_DMFDP, TDK_MFUL, TDK_PTD, TDK_PQD, TDK_DPMEL, TDK_KLAB, TDK_NARR };
#define TDK_MIN_LEVELS 3            /* of the scheme (kte - 1 of the model) */
#define TDK_MAX_LEVELS 128          /* of the scheme; sizes the workspace */

/* what the coverage conditions of tests/test_tiedtke_oracle.py count (host only: TDK_DIAG) */
enum { TDK_D_MIDLEVEL = 1, TDK_D_CLOUD = 2, TDK_D_DOWNDRAFT = 4, TDK_D_MELT = 8, TDK_D_EVAP = 16, TDK_D_ICE = 32, TDK_D_WATER = 64,
       TDK_D_PCTE_WARM = 128, TDK_D_PCTE_COLD = 256, TDK_D_PCTE_MIXED = 512, TDK_D_PRECIP = 1024, TDK_D_SECOND_LOST = 2048,
       TDK_D_MFMAX = 4096 };
#ifdef TDK_DIAG
#define TDK_FLAG(x) (*diag |= (x))
#else
#define TDK_FLAG(x) ((void)0)
#endif

/* Fortran's max / min as this flang lowers them: a compare and a select of the first operand */
#define TDK_MAX(a, b) ((a) > (b) ? (a) : (b))
#define TDK_MIN(a, b) ((a) < (b) ? (a) : (b))

/* cu_tiedtke.f90:25-138 */
#define TDK_T000 273.15f
#define TDK_HGFR 233.15f
#define TDK_ALV 2.5008E6f
#define TDK_ALS 2.8345E6f
#define TDK_ALF (TDK_ALS - TDK_ALV)
#define TDK_CPD 1005.46f
#define TDK_RCPD (1.0f / TDK_CPD)
#define TDK_RHOH2O 1.0E03f
#define TDK_TMELT 273.16f
#define TDK_G 9.806f
#define TDK_ZRG (1.0f / TDK_G)
#define TDK_RD 287.05f
#define TDK_RV 461.51f
#define TDK_C1ES 610.78f
#define TDK_C2ES (TDK_C1ES * TDK_RD / TDK_RV)
#define TDK_C3LES 17.269f
#define TDK_C4LES 35.86f
#define TDK_C5LES (TDK_C3LES * (TDK_TMELT - TDK_C4LES))
#define TDK_C3IES 21.875f
#define TDK_C4IES 7.66f
#define TDK_C5IES (TDK_C3IES * (TDK_TMELT - TDK_C4IES))
#define TDK_VTMPC1 (TDK_RV / TDK_RD - 1.0f)
#define TDK_CEVAPCU1 (1.93E-6f * 261.0f * 0.5f / TDK_G)
#define TDK_CEVAPCU2 (1.E3f / (38.3f * 0.293f))
#define TDK_ENTRSCV 1.2E-3f
#define TDK_ENTRMID 1.0E-4f
#define TDK_ENTRDD 2.0E-4f
#define TDK_CMFCTOP 0.30f
#define TDK_CMFCMAX 1.0f
#define TDK_CMFCMIN 1.E-10f
#define TDK_CMFDEPS 0.30f
#define TDK_CPRCON (1.1E-3f / TDK_G)
#define TDK_ZDNOPRC 1.5E4f
#define TDK_RHC 0.80f
#define TDK_RHM 1.0f
#define TDK_ZBUO0 0.50f
#define TDK_FDBK 1.0f

/* the model's arrays of one column: element k (0-based from the ground) of an array sits at [k * ls]; pint and w have n + 1 levels */
typedef struct {
    const float *t, *qv, *qc, *qi, *pi, *rho, *w, *dz, *p, *pint;
    size_t ls;
} TdkIn;

/* the scalars a column carries from one stage to the next */
typedef struct {
    int kcbot, kctop, ictop0, ktype, ldcum, loddraf, idtop, ilwmin;
    float zmfub, zentr, zrfl, prfl, psfl;
} TdkState;

#define TDK_WS(a, k) ws[((size_t)(a) * nl + (size_t)(k)) * stride]
#define TDK_KLABI(k) ((int)TDK_WS(TDK_KLAB, k))
/* the flip of :399-426: scheme level zz (1 = top) is model level n + 1 - zz; interface zz is model interface n + 2 - zz */
#define TDK_PTEN(zz) in.t[(size_t)(n - (zz)) * in.ls]
#define TDK_PAP(zz) in.p[(size_t)(n - (zz)) * in.ls]
#define TDK_PAPH(zz) in.pint[(size_t)(n + 1 - (zz)) * in.ls]

TDK_FN float tdk_tlucua(float tt)                                                  /* :3470-3487 */
{
    float zcvm3, zcvm4;
    if (tt - TDK_TMELT > 0.f) { zcvm3 = TDK_C3LES; zcvm4 = TDK_C4LES; } else { zcvm3 = TDK_C3IES; zcvm4 = TDK_C4IES; }
    return TDK_C2ES * TDK_EXPF(zcvm3 * (tt - TDK_TMELT) * (1.f / (tt - zcvm4)));
}

TDK_FN float tdk_tlucub(float tt)                                                  /* :3489-3508 */
{
    const float z5alvcp = TDK_C5LES * TDK_ALV / TDK_CPD, z5alscp = TDK_C5IES * TDK_ALS / TDK_CPD;
    float zcvm4, zcvm5;
    if (tt - TDK_TMELT > 0.f) { zcvm4 = TDK_C4LES; zcvm5 = z5alvcp; } else { zcvm4 = TDK_C4IES; zcvm5 = z5alscp; }
    const float r = 1.f / (tt - zcvm4);
    return zcvm5 * (r * r);
}

TDK_FN float tdk_tlucuc(float tt)                                                  /* :3510-3527 */
{
    return tt - TDK_TMELT > 0.f ? TDK_ALV / TDK_CPD : TDK_ALS / TDK_CPD;
}

/* one step of CUADJTQ's adjustment (:3213-3222 and its copies): returns ZCOND before it is clipped and applied */
TDK_FN float tdk_adj_cond(float zqp, float pt, float pq)
{
    float zqsat = tdk_tlucua(pt) * zqp;
    zqsat = TDK_MIN(0.5f, zqsat);
    const float zcor = 1.f / (1.f - TDK_VTMPC1 * zqsat);
    zqsat = zqsat * zcor;
    return (pq - zqsat) / (1.f + zqsat * zcor * tdk_tlucub(pt));
}

/* CUADJTQ (:3170-3325) for one column that has LDFLAG set; kcall 0, 1 or 2 */
TDK_FN void tdk_cuadjtq(float pp, float *ptp, float *pqp, int kcall)
{
    const float zqp = 1.f / pp;
    float pt = *ptp, pq = *pqp;
    float zcond = tdk_adj_cond(zqp, pt, pq);
    if (kcall == 1) zcond = TDK_MAX(zcond, 0.f);
    if (kcall == 2) zcond = TDK_MIN(zcond, 0.f);
    float tt = pt;
    pt = pt + tdk_tlucuc(tt) * zcond;
    pq = pq - zcond;
    if (kcall == 0 || zcond != 0.f) {
        tt = pt;
        const float zcond1 = tdk_adj_cond(zqp, pt, pq);
        pt = pt + tdk_tlucuc(tt) * zcond1;
        pq = pq - zcond1;
    }
    *ptp = pt; *pqp = pq;
}

/* :2098-2106 on the row's first column: the level above which mid-level convection may not start */
TDK_FN int tdk_leveltop(const float *pint, size_t ls, int n)
{
    int leveltop = n - 1;
    for (int jk = n - 1; jk >= 2; jk--) {
        const float d = pint[(size_t)(n + 1 - jk) * ls] * 0.01f - 250.f;
        if ((d < 0.f ? -d : d) < 50.f) { leveltop = jk; break; }
    }
    return TDK_MIN(n - 15, leveltop);
}

/* stage 1: the flip and TIECNV's conversion (:365-441, :626-648), CUINI, CUBASE, CUMASTR_NEW :888-964 */
TDK_FN void tdk_init(TdkIn in, int n, int lndj, float dt, TdkState *s, float *ws, size_t stride, size_t nl, int *diag)
{
    (void)diag;
    const int klev = n, klevm1 = n - 1;
    const float zcons2 = 1.f / (TDK_G * dt);
    /* ZI / ZL (:365-385), DOT (:395), PGEO, ZQP1, ZQSAT */
    {
        float zi = 0.f, zl_prev = 0.f;
        for (int k = 1; k <= n; k++) {                                             /* model order */
            const int zz = n + 1 - k;
            float zl;
            if (k < n) { const float zi1 = zi + in.dz[(size_t)(k - 1) * in.ls]; zl = (zi1 + zi) * 0.5f; zi = zi1; }
            else zl = 2.f * zi - zl_prev;
            zl_prev = zl;
            TDK_WS(TDK_PVERV, zz) = -0.5f * TDK_G * in.rho[(size_t)(k - 1) * in.ls] * (in.w[(size_t)(k - 1) * in.ls] + in.w[(size_t)k * in.ls]);
            TDK_WS(TDK_PGEO, zz) = TDK_G * zl;
            const float q = in.qv[(size_t)(k - 1) * in.ls];
            TDK_WS(TDK_PQEN, zz) = q / (1.0f + q);
            float zqsat = tdk_tlucua(TDK_PTEN(zz)) / TDK_PAP(zz);
            TDK_FLAG(TDK_PTEN(zz) - TDK_TMELT > 0.f ? TDK_D_WATER : TDK_D_ICE);
            zqsat = TDK_MIN(0.5f, zqsat);
            TDK_WS(TDK_PQSEN, zz) = zqsat / (1.f - TDK_VTMPC1 * zqsat);
        }
    }
    /* CUINI :1313-1356 */
    for (int jk = 2; jk <= klev; jk++) {
        TDK_WS(TDK_GEOH, jk) = TDK_WS(TDK_PGEO, jk) + (TDK_WS(TDK_PGEO, jk - 1) - TDK_WS(TDK_PGEO, jk)) * 0.5f;
        const float a = TDK_CPD * TDK_PTEN(jk - 1) + TDK_WS(TDK_PGEO, jk - 1), b = TDK_CPD * TDK_PTEN(jk) + TDK_WS(TDK_PGEO, jk);
        float tenh = (TDK_MAX(a, b) - TDK_WS(TDK_GEOH, jk)) * TDK_RCPD;
        float qsenh = TDK_WS(TDK_PQSEN, jk - 1);
        tdk_cuadjtq(TDK_PAPH(jk), &tenh, &qsenh, 0);
        TDK_WS(TDK_TENH, jk) = tenh;
        TDK_WS(TDK_QSENH, jk) = qsenh;
        float qenh = TDK_MIN(TDK_WS(TDK_PQEN, jk - 1), TDK_WS(TDK_PQSEN, jk - 1)) + (qsenh - TDK_WS(TDK_PQSEN, jk - 1));
        TDK_WS(TDK_QENH, jk) = TDK_MAX(qenh, 0.f);
    }
    TDK_WS(TDK_TENH, klev) = (TDK_CPD * TDK_PTEN(klev) + TDK_WS(TDK_PGEO, klev) - TDK_WS(TDK_GEOH, klev)) * TDK_RCPD;
    TDK_WS(TDK_QENH, klev) = TDK_WS(TDK_PQEN, klev);
    TDK_WS(TDK_TENH, 1) = TDK_PTEN(1);
    TDK_WS(TDK_QENH, 1) = TDK_WS(TDK_PQEN, 1);
    TDK_WS(TDK_GEOH, 1) = TDK_WS(TDK_PGEO, 1);
    TDK_WS(TDK_QSENH, 1) = 0.f;                                                    /* never set and never read in the reference */
    for (int jk = klevm1; jk >= 2; jk--) {
        const float a = TDK_CPD * TDK_WS(TDK_TENH, jk) + TDK_WS(TDK_GEOH, jk), b = TDK_CPD * TDK_WS(TDK_TENH, jk + 1) + TDK_WS(TDK_GEOH, jk + 1);
        const float zzs = TDK_MAX(a, b);
        TDK_WS(TDK_TENH, jk) = (zzs - TDK_WS(TDK_GEOH, jk)) * TDK_RCPD;
    }
    int klwmin = klev;
    float zwmax = 0.f;
    for (int jk = klev; jk >= 3; jk--)
        if (TDK_WS(TDK_PVERV, jk) < zwmax) { zwmax = TDK_WS(TDK_PVERV, jk); klwmin = jk; }
    s->ilwmin = klwmin;
    /* CUINI :1361-1386 */
    for (int jk = 1; jk <= klev; jk++) {
        TDK_WS(TDK_PTU, jk) = TDK_WS(TDK_TENH, jk);
        TDK_WS(TDK_PTD, jk) = TDK_WS(TDK_TENH, jk);
        TDK_WS(TDK_PQU, jk) = TDK_WS(TDK_QENH, jk);
        TDK_WS(TDK_PQD, jk) = TDK_WS(TDK_QENH, jk);
        TDK_WS(TDK_PLU, jk) = 0.f; TDK_WS(TDK_PMFU, jk) = 0.f; TDK_WS(TDK_PMFD, jk) = 0.f; TDK_WS(TDK_MFUS, jk) = 0.f;
        TDK_WS(TDK_MFDS, jk) = 0.f; TDK_WS(TDK_MFUQ, jk) = 0.f; TDK_WS(TDK_MFDQ, jk) = 0.f; TDK_WS(TDK_DMFUP, jk) = 0.f;
        TDK_WS(TDK_DMFDP, jk) = 0.f; TDK_WS(TDK_DPMEL, jk) = 0.f; TDK_WS(TDK_PLUDE, jk) = 0.f; TDK_WS(TDK_MFUL, jk) = 0.f;
        TDK_WS(TDK_KLAB, jk) = 0.f;
    }
    /* CUBASE :1454-1522 */
    TDK_WS(TDK_KLAB, klev) = 1.f;
    int kcbot = klevm1, ldcum = 0;
    for (int jk = klevm1; jk >= 2; jk--) {
        if (TDK_KLABI(jk + 1) != 1) continue;
        float pqu = TDK_WS(TDK_PQU, jk + 1);
        float ptu = (TDK_CPD * TDK_WS(TDK_PTU, jk + 1) + TDK_WS(TDK_GEOH, jk + 1) - TDK_WS(TDK_GEOH, jk)) * TDK_RCPD;
        float zbuo = ptu * (1.f + TDK_VTMPC1 * pqu) - TDK_WS(TDK_TENH, jk) * (1.f + TDK_VTMPC1 * TDK_WS(TDK_QENH, jk)) + TDK_ZBUO0;
        if (zbuo > 0.f) TDK_WS(TDK_KLAB, jk) = 1.f;
        const float zqold = pqu;
        tdk_cuadjtq(TDK_PAPH(jk), &ptu, &pqu, 1);
        TDK_WS(TDK_PTU, jk) = ptu;
        TDK_WS(TDK_PQU, jk) = pqu;
        if (pqu != zqold) {
            TDK_WS(TDK_KLAB, jk) = 2.f;
            TDK_WS(TDK_PLU, jk) = TDK_WS(TDK_PLU, jk) + zqold - pqu;
            zbuo = ptu * (1.f + TDK_VTMPC1 * pqu) - TDK_WS(TDK_TENH, jk) * (1.f + TDK_VTMPC1 * TDK_WS(TDK_QENH, jk)) + TDK_ZBUO0;
            if (zbuo > 0.f) { kcbot = jk; ldcum = 1; }
        }
    }
    /* CUMASTR_NEW :888-950 with PQTE = 0: KTYPE = 2, ZDQPBL = 0, so :931's ELSE */
    (void)ldcum;
    s->ktype = 2;
    s->ldcum = 0;
    {
        const int ikb = kcbot;
        float zmfub = 0.01f;
        const float zmfmax = (TDK_PAPH(ikb) - TDK_PAPH(ikb - 1)) * zcons2;
        s->zmfub = TDK_MIN(zmfub, zmfmax);
    }
    const float zhcbase = TDK_CPD * TDK_WS(TDK_PTU, kcbot) + TDK_WS(TDK_GEOH, kcbot) + TDK_ALV * TDK_WS(TDK_PQU, kcbot);
    int ictop0 = kcbot - 1;
    const float zalvdcp = TDK_ALV / TDK_CPD, zqalv = 1.f / TDK_ALV;
    for (int jk = klevm1; jk >= 3; jk--) {                                         /* :953-964 */
        const float tenh = TDK_WS(TDK_TENH, jk), qsenh = TDK_WS(TDK_QSENH, jk);
        const float zhsat = TDK_CPD * tenh + TDK_WS(TDK_GEOH, jk) + TDK_ALV * qsenh;
        const float d = tenh - TDK_C4LES;
        const float zgam = TDK_C5LES * zalvdcp * qsenh / ((1.f - TDK_VTMPC1 * qsenh) * (d * d));
        const float zzz = TDK_CPD * tenh * 0.608f;
        const float dq = qsenh - TDK_WS(TDK_QENH, jk);
        const float zhhat = zhsat - (zzz + zgam * zzz) / (1.f + zgam * zzz * zqalv) * TDK_MAX(dq, 0.f);
        if (jk < ictop0 && zhcbase > zhhat) ictop0 = jk;
    }
    s->kcbot = kcbot;
    s->ictop0 = ictop0;
    s->kctop = klevm1;
    s->zentr = TDK_ENTRSCV;                                                        /* :1010-1015 with KTYPE = 2 */
    if (lndj == 1) s->zentr = s->zentr * 1.05f;
    s->loddraf = 0; s->idtop = 0; s->zrfl = 0.f; s->prfl = 0.f; s->psfl = 0.f;
}

/* CUASC_NEW (:1882-2382) with CUBASMC and CUENTR_NEW, KTYPE in {0, 3} */
TDK_FN void tdk_ascent(TdkIn in, int n, int leveltop, float dt, TdkState *s, float *ws, size_t stride, size_t nl, int *diag)
{
    const int klev = n, klevm1 = n - 1;
    const float zcons2 = 1.f / (TDK_G * dt);
    int ldcum = s->ldcum, ktype = s->ktype, kcbot = s->kcbot, kctop0 = s->ictop0, kctop;
    float pmfub = s->zmfub, pentr = s->zentr;
    (void)diag;
    if (!ldcum) ktype = 0;                                                         /* :2016 */
    for (int jk = 1; jk <= klev; jk++) {                                           /* :2018-2032 */
        TDK_WS(TDK_PLU, jk) = 0.f; TDK_WS(TDK_PMFU, jk) = 0.f; TDK_WS(TDK_MFUS, jk) = 0.f; TDK_WS(TDK_MFUQ, jk) = 0.f;
        TDK_WS(TDK_MFUL, jk) = 0.f; TDK_WS(TDK_PLUDE, jk) = 0.f; TDK_WS(TDK_DMFUP, jk) = 0.f;
        if (!ldcum || ktype == 3) TDK_WS(TDK_KLAB, jk) = 0.f;
        if (!ldcum && TDK_PAPH(jk) < 4.E4f) kctop0 = jk;
    }
    kctop = klevm1;                                                                /* :2036-2050 */
    if (!ldcum) { kcbot = klevm1; pmfub = 0.f; TDK_WS(TDK_PQU, klev) = 0.f; }
    TDK_WS(TDK_PMFU, klev) = pmfub;
    TDK_WS(TDK_MFUS, klev) = pmfub * (TDK_CPD * TDK_WS(TDK_PTU, klev) + TDK_WS(TDK_GEOH, klev));
    TDK_WS(TDK_MFUQ, klev) = pmfub * TDK_WS(TDK_PQU, klev);
    ldcum = 0;                                                                     /* :2055 */
    const int levelbot = klevm1 - 4;
    for (int jk = klevm1; jk >= 2; jk--) {
        if (jk < levelbot && jk > leveltop) {                                      /* CUBASMC :3136-3162 */
            if (!ldcum && TDK_KLABI(jk + 1) == 0 && TDK_WS(TDK_PQEN, jk) > 0.80f * TDK_WS(TDK_PQSEN, jk)) {
                TDK_WS(TDK_PTU, jk + 1) = (TDK_CPD * TDK_PTEN(jk) + TDK_WS(TDK_PGEO, jk) - TDK_WS(TDK_GEOH, jk + 1)) * TDK_RCPD;
                TDK_WS(TDK_PQU, jk + 1) = TDK_WS(TDK_PQEN, jk);
                TDK_WS(TDK_PLU, jk + 1) = 0.f;
                const float mv = -TDK_WS(TDK_PVERV, jk) / TDK_G;
                float zzzmb = TDK_MAX(TDK_CMFCMIN, mv);
                zzzmb = TDK_MIN(zzzmb, TDK_CMFCMAX);
                pmfub = zzzmb;
                TDK_WS(TDK_PMFU, jk + 1) = pmfub;
                TDK_WS(TDK_MFUS, jk + 1) = pmfub * (TDK_CPD * TDK_WS(TDK_PTU, jk + 1) + TDK_WS(TDK_GEOH, jk + 1));
                TDK_WS(TDK_MFUQ, jk + 1) = pmfub * TDK_WS(TDK_PQU, jk + 1);
                TDK_WS(TDK_MFUL, jk + 1) = 0.f;
                TDK_WS(TDK_DMFUP, jk + 1) = 0.f;
                kcbot = jk;
                TDK_WS(TDK_KLAB, jk + 1) = 1.f;
                ktype = 3;
                pentr = TDK_ENTRMID;
                TDK_FLAG(TDK_D_MIDLEVEL);
            }
        }
        float zqold = 0.0f;                                                        /* :2124-2142 */
        const int klab1 = TDK_KLABI(jk + 1);
        if (klab1 == 0) TDK_WS(TDK_KLAB, jk) = 0.f;
        const int loflag = klab1 > 0;
        if (ktype == 3 && jk == kcbot) {
            const float zmfmax = (TDK_PAPH(jk) - TDK_PAPH(jk - 1)) * zcons2;
            if (pmfub > zmfmax) {
                const float zfac = zmfmax / pmfub;
                TDK_WS(TDK_PMFU, jk + 1) = TDK_WS(TDK_PMFU, jk + 1) * zfac;
                TDK_WS(TDK_MFUS, jk + 1) = TDK_WS(TDK_MFUS, jk + 1) * zfac;
                TDK_WS(TDK_MFUQ, jk + 1) = TDK_WS(TDK_MFUQ, jk + 1) * zfac;
                pmfub = zmfmax;
                TDK_FLAG(TDK_D_MFMAX);
            }
        }
        if (!loflag) continue;
        /* CUENTR_NEW :3382-3440 with nturben = 1 (fscale = 1) */
        const float paph_k = TDK_PAPH(jk), paph_k1 = TDK_PAPH(jk + 1);
        const float zpbase = TDK_PAPH(kcbot);
        float zdmfen, zdmfde;
        {
            const float zrrho = (TDK_RD * TDK_WS(TDK_TENH, jk + 1)) / paph_k1;
            const float zdprho = (paph_k1 - paph_k) * TDK_ZRG;
            const float zpmid = 0.5f * (zpbase + TDK_PAPH(kctop0));
            const float zentr = pentr * TDK_WS(TDK_PMFU, jk + 1) * zdprho * zrrho;
            const int llo1 = jk < kcbot && ldcum;
            zdmfde = llo1 ? zentr : 0.0f;
            zdmfen = 0.0f;
            const int iklwmin = TDK_MAX(s->ilwmin, kctop0 + 2);
            if (llo1 && ktype == 3 && (jk >= iklwmin || TDK_PAP(jk) > zpmid)) zdmfen = zentr * 1.0f;
        }
        float zoentr = 0.f, zodetr = 0.f;                                          /* ZOENTR(JL,JK), ZODETR(JL,JK): +0 unless KTYPE = 1 */
        const float pmfu1 = TDK_WS(TDK_PMFU, jk + 1);
        if (jk < kcbot) {                                                          /* :2165-2169 */
            const float zmftest = pmfu1 + zdmfen - zdmfde;
            const float lim = (paph_k - TDK_PAPH(jk - 1)) * zcons2;
            const float zmfmax = TDK_MIN(zmftest, lim);
            const float ex = zmftest - zmfmax;
            const float v = zdmfen - TDK_MAX(ex, 0.f);
            zdmfen = TDK_MAX(v, 0.f);
        }
        { const float lim = 0.75f * pmfu1; zdmfde = TDK_MIN(zdmfde, lim); }
        float pmfu = pmfu1 + zdmfen - zdmfde;
        if (jk < kcbot) {                                                          /* :2172-2178 */
            const float zdprho = (TDK_WS(TDK_GEOH, jk) - TDK_WS(TDK_GEOH, jk + 1)) * TDK_ZRG;
            zoentr = zoentr * zdprho * pmfu1;
            const float zmftest = pmfu + zoentr - zodetr;
            const float lim = (paph_k - TDK_PAPH(jk - 1)) * zcons2;
            const float zmfmax = TDK_MIN(zmftest, lim);
            const float ex = zmftest - zmfmax;
            const float v = zoentr - TDK_MAX(ex, 0.f);
            zoentr = TDK_MAX(v, 0.f);
        }
        { const float lim = 0.75f * pmfu; zodetr = TDK_MIN(zodetr, lim); }
        pmfu = pmfu + zoentr - zodetr;
        const float qenh1 = TDK_WS(TDK_QENH, jk + 1), tenh1 = TDK_WS(TDK_TENH, jk + 1), geoh1 = TDK_WS(TDK_GEOH, jk + 1);
        const float qsenh1 = TDK_WS(TDK_QSENH, jk + 1), plu1 = TDK_WS(TDK_PLU, jk + 1);
        float zqeen = qenh1 * zdmfen;
        zqeen = zqeen + qenh1 * zoentr;
        float zseen = (TDK_CPD * tenh1 + geoh1) * zdmfen;
        zseen = zseen + (TDK_CPD * tenh1 + geoh1) * zoentr;
        float zscde = (TDK_CPD * TDK_WS(TDK_PTU, jk + 1) + geoh1) * zdmfde;
        const float zga = TDK_ALV * qsenh1 / (TDK_RV * (tenh1 * tenh1));
        const float zdt = (plu1 - 0.608f * (qsenh1 - qenh1)) / (1.f / tenh1 + 0.608f * zga);
        const float zscod = TDK_CPD * tenh1 + geoh1 + TDK_CPD * zdt;
        zscde = zscde + zodetr * zscod;
        float zqude = TDK_WS(TDK_PQU, jk + 1) * zdmfde;
        const float zqcod = qsenh1 + zga * zdt;
        zqude = zqude + zodetr * zqcod;
        float plude = plu1 * zdmfde;
        plude = plude + plu1 * zodetr;
        TDK_WS(TDK_PLUDE, jk) = plude;
        const float zmfusk = TDK_WS(TDK_MFUS, jk + 1) + zseen - zscde;
        const float zmfuqk = TDK_WS(TDK_MFUQ, jk + 1) + zqeen - zqude;
        const float zmfulk = TDK_WS(TDK_MFUL, jk + 1) - plude;
        const float rm = 1.f / TDK_MAX(TDK_CMFCMIN, pmfu);
        float plu = zmfulk * rm;
        float pqu = zmfuqk * rm;
        float ptu = (zmfusk * rm - TDK_WS(TDK_GEOH, jk)) * TDK_RCPD;
        ptu = TDK_MAX(100.f, ptu);
        ptu = TDK_MIN(400.f, ptu);
        zqold = pqu;
        tdk_cuadjtq(paph_k, &ptu, &pqu, 1);                                        /* :2230 */
        if (pqu != zqold) {                                                        /* :2233-2255 */
            TDK_WS(TDK_KLAB, jk) = 2.f;
            plu = plu + zqold - pqu;
            float zbuo = ptu * (1.f + TDK_VTMPC1 * pqu - plu) - TDK_WS(TDK_TENH, jk) * (1.f + TDK_VTMPC1 * TDK_WS(TDK_QENH, jk));
            if (klab1 == 1) zbuo = zbuo + TDK_ZBUO0;
            if (zbuo > 0.f && pmfu > 0.01f * pmfub && jk >= kctop0) {
                kctop = jk;
                ldcum = 1;
                const float zprcon = (zpbase - paph_k >= TDK_ZDNOPRC) ? TDK_CPRCON : 0.f;
                const float zlnew = plu / (1.f + zprcon * (TDK_WS(TDK_GEOH, jk) - TDK_WS(TDK_GEOH, jk + 1)));
                const float dm = (plu - zlnew) * pmfu;
                TDK_WS(TDK_DMFUP, jk) = TDK_MAX(0.f, dm);
                plu = zlnew;
                TDK_FLAG(TDK_D_CLOUD);
            } else {
                TDK_WS(TDK_KLAB, jk) = 0.f;
                pmfu = 0.f;
            }
        }
        TDK_WS(TDK_PLU, jk) = plu; TDK_WS(TDK_PQU, jk) = pqu; TDK_WS(TDK_PTU, jk) = ptu; TDK_WS(TDK_PMFU, jk) = pmfu;
        TDK_WS(TDK_MFUL, jk) = plu * pmfu;                                         /* :2256-2260 */
        TDK_WS(TDK_MFUS, jk) = (TDK_CPD * ptu + TDK_WS(TDK_GEOH, jk)) * pmfu;
        TDK_WS(TDK_MFUQ, jk) = pqu * pmfu;
    }
    if (kctop == klevm1) ldcum = 0;                                                /* :2341-2344 */
    kcbot = TDK_MAX(kcbot, kctop);
    if (ldcum) {                                                                   /* :2353-2370 */
        const int jk = kctop - 1;
        const float zdmfde = (1.f - TDK_CMFCTOP) * TDK_WS(TDK_PMFU, jk + 1);
        TDK_WS(TDK_PLUDE, jk) = zdmfde * TDK_WS(TDK_PLU, jk + 1);
        const float pmfu = TDK_WS(TDK_PMFU, jk + 1) - zdmfde;
        TDK_WS(TDK_PMFU, jk) = pmfu;
        TDK_WS(TDK_MFUS, jk) = (TDK_CPD * TDK_WS(TDK_PTU, jk) + TDK_WS(TDK_GEOH, jk)) * pmfu;
        TDK_WS(TDK_MFUQ, jk) = TDK_WS(TDK_PQU, jk) * pmfu;
        TDK_WS(TDK_MFUL, jk) = TDK_WS(TDK_PLU, jk) * pmfu;
        if (jk == 1) TDK_WS(TDK_PLUDE, jk) = TDK_WS(TDK_MFUL, jk);
        else TDK_WS(TDK_PLUDE, jk - 1) = TDK_WS(TDK_MFUL, jk);
        TDK_WS(TDK_DMFUP, jk) = 0.f;
    }
    s->ldcum = ldcum; s->ktype = ktype; s->kcbot = kcbot; s->kctop = kctop; s->ictop0 = kctop0; s->zmfub = pmfub; s->zentr = pentr;
}

/* CUMASTR_NEW :1033-1188 between the two ascents: the precipitation of the first ascent, CUDLFS, CUDDRAF, the closure for KTYPE /= 1 */
TDK_FN void tdk_downdraft(TdkIn in, int n, float dt, TdkState *s, float *ws, size_t stride, size_t nl, int *diag)
{
    const int klev = n;
    const float zcons2 = 1.f / (TDK_G * dt);
    const int ldcum = s->ldcum, kcbot = s->kcbot, kctop = s->kctop;
    (void)diag;
    if (ldcum) s->ictop0 = kctop;                                                  /* :1035 */
    float zrfl = TDK_WS(TDK_DMFUP, 1);
    for (int jk = 2; jk <= klev; jk++) zrfl = zrfl + TDK_WS(TDK_DMFUP, jk);
    /* CUDLFS :2443-2521 */
    int lddraf = 0, kdtop = klev + 1;
    for (int jk = 3; jk <= klev - 3; jk++) {
        const int llo2 = ldcum && zrfl > 0.f && !lddraf && (jk < kcbot && jk > kctop);
        if (!llo2) continue;
        float ztenwb = TDK_WS(TDK_TENH, jk), zqenwb = TDK_WS(TDK_QENH, jk);
        tdk_cuadjtq(TDK_PAPH(jk), &ztenwb, &zqenwb, 2);
        const float zttest = 0.5f * (TDK_WS(TDK_PTU, jk) + ztenwb);
        const float zqtest = 0.5f * (TDK_WS(TDK_PQU, jk) + zqenwb);
        const float zbuo = zttest * (1.f + TDK_VTMPC1 * zqtest) - TDK_WS(TDK_TENH, jk) * (1.f + TDK_VTMPC1 * TDK_WS(TDK_QENH, jk));
        const float zcond = TDK_WS(TDK_QENH, jk) - zqenwb;
        const float zmftop = -TDK_CMFDEPS * s->zmfub;
        if (zbuo < 0.f && zrfl > 10.f * zmftop * zcond) {
            kdtop = jk;
            lddraf = 1;
            TDK_WS(TDK_PTD, jk) = zttest;
            TDK_WS(TDK_PQD, jk) = zqtest;
            TDK_WS(TDK_PMFD, jk) = zmftop;
            TDK_WS(TDK_MFDS, jk) = zmftop * (TDK_CPD * zttest + TDK_WS(TDK_GEOH, jk));
            TDK_WS(TDK_MFDQ, jk) = zmftop * zqtest;
            TDK_WS(TDK_DMFDP, jk - 1) = -0.5f * zmftop * zcond;
            zrfl = zrfl + TDK_WS(TDK_DMFDP, jk - 1);
            TDK_FLAG(TDK_D_DOWNDRAFT);
        }
    }
    /* CUDDRAF :2588-2664 */
    for (int jk = 3; jk <= klev; jk++) {
        const float pmfd1 = TDK_WS(TDK_PMFD, jk - 1);
        if (!(lddraf && pmfd1 < 0.f)) continue;
        const float paph_k = TDK_PAPH(jk), paph_k1 = TDK_PAPH(jk - 1);
        const float zentr = TDK_ENTRDD * pmfd1 * TDK_RD * TDK_WS(TDK_TENH, jk - 1) / (TDK_G * paph_k1) * (paph_k - paph_k1);
        float zdmfen = zentr, zdmfde = zentr;
        const int itopde = klev - 2;
        if (jk > itopde) {
            zdmfen = 0.f;
            zdmfde = TDK_WS(TDK_PMFD, itopde) * (paph_k - paph_k1) / (TDK_PAPH(klev + 1) - TDK_PAPH(itopde));
        }
        float pmfd = pmfd1 + zdmfen - zdmfde;
        const float se = TDK_CPD * TDK_WS(TDK_TENH, jk - 1) + TDK_WS(TDK_GEOH, jk - 1);
        const float zseen = se * zdmfen;
        const float zqeen = TDK_WS(TDK_QENH, jk - 1) * zdmfen;
        const float zsdde = (TDK_CPD * TDK_WS(TDK_PTD, jk - 1) + TDK_WS(TDK_GEOH, jk - 1)) * zdmfde;
        const float zqdde = TDK_WS(TDK_PQD, jk - 1) * zdmfde;
        const float zmfdsk = TDK_WS(TDK_MFDS, jk - 1) + zseen - zsdde;
        const float zmfdqk = TDK_WS(TDK_MFDQ, jk - 1) + zqeen - zqdde;
        const float rm = 1.f / TDK_MIN(-TDK_CMFCMIN, pmfd);
        float pqd = zmfdqk * rm;
        float ptd = (zmfdsk * rm - TDK_WS(TDK_GEOH, jk)) * TDK_RCPD;
        ptd = TDK_MIN(400.f, ptd);
        ptd = TDK_MAX(100.f, ptd);
        float zcond = pqd;
        tdk_cuadjtq(paph_k, &ptd, &pqd, 2);
        zcond = zcond - pqd;
        const float zbuo = ptd * (1.f + TDK_VTMPC1 * pqd) - TDK_WS(TDK_TENH, jk) * (1.f + TDK_VTMPC1 * TDK_WS(TDK_QENH, jk));
        if (zbuo >= 0.f || zrfl <= (pmfd * zcond)) pmfd = 0.f;
        TDK_WS(TDK_PTD, jk) = ptd; TDK_WS(TDK_PQD, jk) = pqd; TDK_WS(TDK_PMFD, jk) = pmfd;
        TDK_WS(TDK_MFDS, jk) = (TDK_CPD * ptd + TDK_WS(TDK_GEOH, jk)) * pmfd;
        TDK_WS(TDK_MFDQ, jk) = pqd * pmfd;
        const float zdmfdp = -pmfd * zcond;
        TDK_WS(TDK_DMFDP, jk - 1) = zdmfdp;
        zrfl = zrfl + zdmfdp;
    }
    /* :1142-1188 with KTYPE /= 1, ZDQPBL = 0 and LLO1 false (KTYPE /= 2): ZMFUB1 = MIN(ZMFUB, ZMFMAX) */
    float zmfub = s->zmfub, zmfub1;
    {
        const int ikb = kcbot;
        const float zmfmax = (TDK_PAPH(ikb) - TDK_PAPH(ikb - 1)) * zcons2;
        zmfub1 = zmfub;
        zmfub1 = TDK_MIN(zmfub1, zmfmax);
    }
    if (ldcum) {
        const float zfac = zmfub1 / TDK_MAX(zmfub, 1.E-10f);
        for (int jk = 1; jk <= klev; jk++) {
            TDK_WS(TDK_PMFD, jk) = TDK_WS(TDK_PMFD, jk) * zfac;
            TDK_WS(TDK_MFDS, jk) = TDK_WS(TDK_MFDS, jk) * zfac;
            TDK_WS(TDK_MFDQ, jk) = TDK_WS(TDK_MFDQ, jk) * zfac;
            TDK_WS(TDK_DMFDP, jk) = TDK_WS(TDK_DMFDP, jk) * zfac;
        }
        zmfub = zmfub1;
    } else {
        for (int jk = 1; jk <= klev; jk++) {
            TDK_WS(TDK_PMFD, jk) = 0.f; TDK_WS(TDK_MFDS, jk) = 0.f; TDK_WS(TDK_MFDQ, jk) = 0.f; TDK_WS(TDK_DMFDP, jk) = 0.f;
        }
        zmfub = 0.f;
    }
    s->zmfub = zmfub; s->zrfl = zrfl; s->loddraf = lddraf; s->idtop = kdtop;
}

/* CUFLX (:2672-2840); KTOPM2 is the column's own (the row's minimum only adds levels on which every flux is zero) */
TDK_FN int tdk_cuflx(TdkIn in, int n, const float *sig1, size_t sig_stride, float dt, TdkState *s, float *ws, size_t stride, size_t nl, int *diag)
{
    const int klev = n;
    const float zcons1 = TDK_CPD / (TDK_ALF * TDK_G * dt), zcons2 = 1.f / (TDK_G * dt), zcucov = 0.05f, ztmelp2 = TDK_TMELT + 2.f;
    const int ldcum = s->ldcum, kcbot = s->kcbot, kctop = s->kctop, kdtop = s->idtop;
    int lddraf = s->loddraf;
    float prfl = 0.f, psfl = 0.f;
    (void)diag;
    if (!ldcum || kdtop < kctop) lddraf = 0;
    if (!ldcum) s->ktype = 0;
    int ktopm2 = kctop - 2;
    if (ktopm2 == 0) ktopm2 = 1;
    for (int jk = ktopm2; jk <= klev; jk++) {                                      /* :2739-2772 */
        if (ldcum && jk >= kctop - 1) {
            const float se = TDK_CPD * TDK_WS(TDK_TENH, jk) + TDK_WS(TDK_GEOH, jk);
            TDK_WS(TDK_MFUS, jk) = TDK_WS(TDK_MFUS, jk) - TDK_WS(TDK_PMFU, jk) * se;
            TDK_WS(TDK_MFUQ, jk) = TDK_WS(TDK_MFUQ, jk) - TDK_WS(TDK_PMFU, jk) * TDK_WS(TDK_QENH, jk);
            if (lddraf && jk >= kdtop) {
                TDK_WS(TDK_MFDS, jk) = TDK_WS(TDK_MFDS, jk) - TDK_WS(TDK_PMFD, jk) * se;
                TDK_WS(TDK_MFDQ, jk) = TDK_WS(TDK_MFDQ, jk) - TDK_WS(TDK_PMFD, jk) * TDK_WS(TDK_QENH, jk);
            } else {
                TDK_WS(TDK_PMFD, jk) = 0.f; TDK_WS(TDK_MFDS, jk) = 0.f; TDK_WS(TDK_MFDQ, jk) = 0.f;
                if (jk > 1) TDK_WS(TDK_DMFDP, jk - 1) = 0.f;
            }
        } else {
            TDK_WS(TDK_PMFU, jk) = 0.f; TDK_WS(TDK_PMFD, jk) = 0.f; TDK_WS(TDK_MFUS, jk) = 0.f; TDK_WS(TDK_MFDS, jk) = 0.f;
            TDK_WS(TDK_MFUQ, jk) = 0.f; TDK_WS(TDK_MFDQ, jk) = 0.f; TDK_WS(TDK_MFUL, jk) = 0.f;
            if (jk > 1) { TDK_WS(TDK_DMFUP, jk - 1) = 0.f; TDK_WS(TDK_DMFDP, jk - 1) = 0.f; TDK_WS(TDK_PLUDE, jk - 1) = 0.f; }
        }
    }
    if (ldcum) for (int jk = ktopm2; jk <= klev; jk++) {                           /* :2773-2807 */
        if (jk > kcbot) {
            const int ikb = kcbot;
            float zzp = (TDK_PAPH(klev + 1) - TDK_PAPH(jk)) / (TDK_PAPH(klev + 1) - TDK_PAPH(ikb));
            if (s->ktype == 3) zzp = zzp * zzp;
            TDK_WS(TDK_PMFU, jk) = TDK_WS(TDK_PMFU, ikb) * zzp;
            TDK_WS(TDK_MFUS, jk) = TDK_WS(TDK_MFUS, ikb) * zzp;
            TDK_WS(TDK_MFUQ, jk) = TDK_WS(TDK_MFUQ, ikb) * zzp;
            TDK_WS(TDK_MFUL, jk) = TDK_WS(TDK_MFUL, ikb) * zzp;
        }
        const float pten = TDK_PTEN(jk);
        if (pten > TDK_TMELT) {
            prfl = prfl + TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk);
            if (psfl > 0.f && pten > ztmelp2) {
                const float zfac = zcons1 * (TDK_PAPH(jk + 1) - TDK_PAPH(jk));
                const float lim = zfac * (pten - ztmelp2);
                const float zsnmlt = TDK_MIN(psfl, lim);
                TDK_WS(TDK_DPMEL, jk) = zsnmlt;
                psfl = psfl - zsnmlt;
                prfl = prfl + zsnmlt;
                if (zsnmlt != 0.f) TDK_FLAG(TDK_D_MELT);
            }
        } else {
            psfl = psfl + TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk);
        }
    }
    prfl = TDK_MAX(prfl, 0.f);                                                     /* :2808-2812 */
    psfl = TDK_MAX(psfl, 0.f);
    float zpsubcl = prfl + psfl;
    if (ldcum) for (int jk = ktopm2; jk <= klev; jk++) {                           /* :2813-2831 */
        if (jk >= kcbot && zpsubcl > 1.E-20f) {
            const float zrfl = zpsubcl;
            const float cevapcu = TDK_CEVAPCU1 * TDK_SQRTF(TDK_CEVAPCU2 * TDK_SQRTF(sig1[(size_t)(n - jk) * sig_stride]));
            const float dp = TDK_PAPH(jk + 1) - TDK_PAPH(jk);
            const float dq = TDK_WS(TDK_PQSEN, jk) - TDK_WS(TDK_PQEN, jk);
            const float r = TDK_SQRTF(zrfl / zcucov) - cevapcu * dp * TDK_MAX(0.f, dq);
            const float rr = TDK_MAX(0.f, r);
            float zrnew = rr * rr * zcucov;
            const float dq8 = 0.8f * TDK_WS(TDK_PQSEN, jk) - TDK_WS(TDK_PQEN, jk);
            const float zrmin = zrfl - zcucov * TDK_MAX(0.f, dq8) * zcons2 * dp;
            zrnew = TDK_MAX(zrnew, zrmin);
            const float zrfln = TDK_MAX(zrnew, 0.f);
            const float dr = zrfln - zrfl;
            const float zdrfl = TDK_MIN(0.f, dr);
            TDK_WS(TDK_DMFUP, jk) = TDK_WS(TDK_DMFUP, jk) + zdrfl;
            zpsubcl = zrfln;
            if (zdrfl != 0.f) TDK_FLAG(TDK_D_EVAP);
        }
    }
    {                                                                              /* :2832-2838 */
        const float zdpevap = zpsubcl - (prfl + psfl);
        const float t1 = prfl + psfl;
        prfl = prfl + zdpevap * prfl * (1.f / TDK_MAX(1.E-20f, t1));
        const float t2 = prfl + psfl;
        psfl = psfl + zdpevap * psfl * (1.f / TDK_MAX(1.E-20f, t2));
    }
    s->prfl = prfl; s->psfl = psfl; s->loddraf = lddraf;
    return ktopm2;
}

/* CUDTDQ (:2846-2968), TIECNV's tail (:666-700) and CU_TIEDTKE's tendencies (:446-485), level by level.  conv = 0: the column
 * left the scheme without convection (every tendency of CUDTDQ is zero). */
TDK_FN float tdk_finish(TdkIn in, int n, int conv, int ktopm2, float dt, const TdkState *s, const float *ws, size_t stride, size_t nl,
                        float *tend_th, float *tend_qv, float *tend_qc, float *tend_qi, size_t os, int *diag)
{
    const int klev = n;
    const float ztmst = dt, rdelt = 1.f / dt;
    (void)diag;
    for (int jk = 1; jk <= klev; jk++) {
        float ptte = 0.0f, pqte = 0.0f, pcte = 0.0f;
        const float pten = TDK_PTEN(jk);
        if (conv && s->ldcum && jk >= ktopm2) {
            const float zalv = pten > TDK_TMELT ? TDK_ALV : TDK_ALS;
            const float rh = TDK_WS(TDK_PQEN, jk) / TDK_WS(TDK_PQSEN, jk);
            const float rhk = TDK_MIN(1.0f, rh);
            const float rc = (rhk - TDK_RHC) / (TDK_RHM - TDK_RHC);
            const float rhcoe = TDK_MAX(0.0f, rc);
            const float pl = rhcoe * TDK_FDBK * TDK_WS(TDK_PLUDE, jk);
            const float pldfd = TDK_MAX(0.0f, pl);
            const float gdp = TDK_G / (TDK_PAPH(jk + 1) - TDK_PAPH(jk));
            float zdtdt, zdqdt;
            if (jk < klev) {
                zdtdt = gdp * TDK_RCPD * (TDK_WS(TDK_MFUS, jk + 1) - TDK_WS(TDK_MFUS, jk) + TDK_WS(TDK_MFDS, jk + 1) - TDK_WS(TDK_MFDS, jk)
                                          - TDK_ALF * TDK_WS(TDK_DPMEL, jk)
                                          - zalv * (TDK_WS(TDK_MFUL, jk + 1) - TDK_WS(TDK_MFUL, jk) - pldfd
                                                    - (TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk))));
                zdqdt = gdp * (TDK_WS(TDK_MFUQ, jk + 1) - TDK_WS(TDK_MFUQ, jk) + TDK_WS(TDK_MFDQ, jk + 1) - TDK_WS(TDK_MFDQ, jk)
                               + TDK_WS(TDK_MFUL, jk + 1) - TDK_WS(TDK_MFUL, jk) - pldfd - (TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk)));
            } else {
                zdtdt = -gdp * TDK_RCPD * (TDK_WS(TDK_MFUS, jk) + TDK_WS(TDK_MFDS, jk) + TDK_ALF * TDK_WS(TDK_DPMEL, jk)
                                           - zalv * (TDK_WS(TDK_MFUL, jk) + TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk) + pldfd));
                zdqdt = -gdp * (TDK_WS(TDK_MFUQ, jk) + TDK_WS(TDK_MFDQ, jk) + pldfd
                                + (TDK_WS(TDK_MFUL, jk) + TDK_WS(TDK_DMFUP, jk) + TDK_WS(TDK_DMFDP, jk)));
            }
            ptte = ptte + zdtdt;
            pqte = pqte + zdqdt;
            pcte = gdp * pldfd;
        }
        const size_t m = (size_t)(n - jk);                                         /* model level, 0-based */
        float pqc = in.qc[m * in.ls], pqi = in.qi[m * in.ls];
        if (pcte > 0.0f) {                                                         /* :669-686 */
            const float ztpp1 = pten + ptte * ztmst;
            float fliq, zalf;
            if (ztpp1 >= TDK_T000) { fliq = 1.0f; zalf = 0.0f; TDK_FLAG(TDK_D_PCTE_WARM); }
            else if (ztpp1 <= TDK_HGFR) { fliq = 0.0f; zalf = TDK_ALF; TDK_FLAG(TDK_D_PCTE_COLD); }
            else {
                const float ztc = ztpp1 - TDK_T000;
                fliq = 0.0059f + 0.9941f * TDK_EXPF(-0.003102f * ztc * ztc);
                zalf = TDK_ALF;
                TDK_FLAG(TDK_D_PCTE_MIXED);
            }
            const float fice = 1.0f - fliq;
            pqc = pqc + fliq * pcte * ztmst;
            pqi = pqi + fice * pcte * ztmst;
            ptte = ptte - zalf * TDK_RCPD * fliq * pcte;
        }
        const float pt = pten + ptte * ztmst;                                      /* :693-695 */
        const float zqp1 = TDK_WS(TDK_PQEN, jk) + (pqte - 0.0f) * ztmst;
        const float pqv = zqp1 / (1.0f - zqp1);
        tend_th[m * os] = (pt - pten) / in.pi[m * in.ls] * rdelt;                  /* :454-481 */
        tend_qv[m * os] = (pqv - in.qv[m * in.ls]) * rdelt;
        tend_qc[m * os] = (pqc - in.qc[m * in.ls]) * rdelt;
        tend_qi[m * os] = (pqi - in.qi[m * in.ls]) * rdelt;
    }
    const float pr = (s->prfl + s->psfl) * ztmst;                                  /* :699 */
    return TDK_MAX(0.0f, pr);
}

/* the whole scheme on one column: the four tendencies (element k at [k * os]), the precipitation RN and the final KTYPE */
TDK_FN float tdk_column(TdkIn in, int n, int lndj, int leveltop, const float *sig1, size_t sig_stride, float dt, float *ws, size_t stride,
                        size_t nl, float *tend_th, float *tend_qv, float *tend_qc, float *tend_qi, size_t os, int *ktype, int *diag)
{
    TdkState s;
    tdk_init(in, n, lndj, dt, &s, ws, stride, nl, diag);
    tdk_ascent(in, n, leveltop, dt, &s, ws, stride, nl, diag);
    int conv = s.ldcum, ktopm2 = 1;
    if (conv) {                                                                    /* ICUM = 0 (:1029) per column */
        tdk_downdraft(in, n, dt, &s, ws, stride, nl, diag);
        tdk_ascent(in, n, leveltop, dt, &s, ws, stride, nl, diag);
#ifdef TDK_DIAG
        if (!s.ldcum) TDK_FLAG(TDK_D_SECOND_LOST);
#endif
        ktopm2 = tdk_cuflx(in, n, sig1, sig_stride, dt, &s, ws, stride, nl, diag);
    } else {
        s.ktype = 0; s.prfl = 0.f; s.psfl = 0.f;
    }
    const float rn = tdk_finish(in, n, conv, ktopm2, dt, &s, ws, stride, nl, tend_th, tend_qv, tend_qc, tend_qi, os, diag);
#ifdef TDK_DIAG
    if (rn > 0.f) TDK_FLAG(TDK_D_PRECIP);
#endif
    *ktype = s.ktype;
    return rn;
}

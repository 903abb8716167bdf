// icar_amd/csrc/bmj_column.h -- one column of the Betts-Miller-Janjic convection scheme, for the device (cu_bmj.hip) and for the
// host (tests/support/bmj_oracle.c compiles this very file with a C compiler; cu_bmj.hip builds the tables with it).
//
// Reference algorithm: src/physics/cu_bmj.f90 -- BMJDRV :78-389 (the column set-up :195-221 and the outputs :245-265), BMJ :393-1739,
// TTBLEX :1743-1819, BMJINIT :1822-2086, SPLINE :2090-2198, with the constants of src/constants/wrf_constants.f90 and the arguments
// src/physics/cu_driver.f90:434-465 passes (cp = 1012, r_d = 287, xlv, gravity, svpt0, EP1 = Rw/Rd - 1).  REAL(4) in the reference's
// operation order; ** and exp are the C library's powf / expf (the includer names them: BMJ_POWF, BMJ_EXPF); every PARAMETER
// expression is written out as the reference writes it, so that the compiler folds it in REAL(4) as flang does.
//
// NOT built: the bmj_rad_feedback block (:267-351: CCLDFRA, QCCONV, QICONV, CONVCLD, PRATEC).  Those arrays are private to
// cu_driver.f90 and nothing reads them; the block needs GAMMA() in REAL(4).  DQCOL, PWCOL and DQCOLMIN feed only that block.
//
// The level arrays of a column live in a workspace laid out [array][level][column]: BMJ_WS(a, L) is level L (1-based, counted from
// the model top as the scheme counts) of array a; `stride` is the number of columns the workspace holds (1 on the host).  What the
// reference keeps in further arrays is not stored: EL (ELWV on every branch), THES / THEScnv (THESP of the trial parcel on every
// level, the entrainment being commented out), TK / QK / PK / APEK (copies of T, Q, PRSMID, APE), FPK (equal to TREFK where it is
// read), QSATK and TREF (consumed where they are made), THVREF's initial profile (made where it is read, at LTOP-1).  CPEcnv /
// DTVcnv are the other half of a pair of arrays that swap roles instead of being copied.
//
// Accesses the reference makes outside its arrays, and what happens here:
//   APEK(L-1), THERK(L-1) with L = LTOP = 1 (:1011-1012)   read and never used: not read here
//   PRSMID(LBOT+1), T(LBOT+1) with LBOT = LMH (:755-767)     reached when no level above the lowest lies PONE = 2500 Pa below it
//                                                            (always with one level: cu_bmj.hip refuses that; otherwise a column
//                                                            thinner than 25 hPa): the trial parcel is given no CAPE here
#pragma once
#include <stddef.h>

#ifndef BMJ_FN
#define BMJ_FN static inline
#endif

enum { BMJ_ITB = 76, BMJ_JTB = 134, BMJ_ITBQ = 152, BMJ_JTBQ = 440 };
enum { BMJ_T = 0, BMJ_Q, BMJ_P, BMJ_DP, BMJ_APE, BMJ_CPE0, BMJ_DTV0, BMJ_CPE1, BMJ_DTV1, BMJ_THERK, BMJ_TREFK, BMJ_QREFK, BMJ_PSK,
       BMJ_APESK, BMJ_DIFT, BMJ_DIFQ, BMJ_NARR, BMJ_THVREF = BMJ_THERK, BMJ_SEARCH_ARRAYS = BMJ_THERK };
enum { BMJ_NONE = 0, BMJ_DEEP = 1, BMJ_SHALLOW = 2 };
#define BMJ_MAX_LEVELS 128          /* of the scheme (kte - kts); sizes the workspace */

typedef struct BmjTables { const float *QS0, *SQS, *PTBL, *THE0, *STHE, *TTBL, *THE0Q, *STHEQ, *TTBLQ; } BmjTables;
#define BMJ_TABLE_FLOATS (2 * BMJ_JTB + BMJ_ITB * BMJ_JTB + 2 * BMJ_ITB + BMJ_JTB * BMJ_ITB + 2 * BMJ_ITBQ + BMJ_JTBQ * BMJ_ITBQ)
/* the nine tables in one block of BMJ_TABLE_FLOATS floats, in this order, each in Fortran element order */
BMJ_FN BmjTables bmj_tables_at(const float *block)
{
    BmjTables tb;
    tb.QS0 = block; tb.SQS = tb.QS0 + BMJ_JTB; tb.PTBL = tb.SQS + BMJ_JTB; tb.THE0 = tb.PTBL + BMJ_ITB * BMJ_JTB; tb.STHE = tb.THE0 + BMJ_ITB;
    tb.TTBL = tb.STHE + BMJ_ITB; tb.THE0Q = tb.TTBL + BMJ_JTB * BMJ_ITB; tb.STHEQ = tb.THE0Q + BMJ_ITBQ; tb.TTBLQ = tb.STHEQ + BMJ_ITBQ;
    return tb;
}

/* module parameters, cu_bmj.f90:15-71, :476-490; wrf_constants.f90:95-100 */
#define BMJ_EFIFC 5.0f
#define BMJ_EFIMN 0.20f
#define BMJ_EFMNT 0.70f
#define BMJ_ELIWV 2.683E6f
#define BMJ_EPSNTP .0001f
#define BMJ_EPSPR 1.E-7f
#define BMJ_EPSDN 1.05f
#define BMJ_EPSDT 0.f
#define BMJ_FR 1.00f
#define BMJ_FSL 0.85f
#define BMJ_FSS 0.85f
#define BMJ_PFRZ 15000.f
#define BMJ_PNO 1000.f
#define BMJ_PONE 2500.f
#define BMJ_PQM 20000.f
#define BMJ_PSH 20000.f
#define BMJ_PSHU 45000.f
#define BMJ_RHLSC 0.00f
#define BMJ_RHHSC 1.10f
#define BMJ_ROW 1.E3f
#define BMJ_STABDF 0.90f
#define BMJ_STABDS 0.90f
#define BMJ_STABS 1.0f
#define BMJ_DTSHAL (-1.0f)
#define BMJ_TREL 2400.f
#define BMJ_DTTRIGR (-0.0f)
#define BMJ_DTPTRIGR (BMJ_DTTRIGR * BMJ_PONE)
#define BMJ_DSPBFL (-3875.f * BMJ_FR)
#define BMJ_DSP0FL (-5875.f * BMJ_FR)
#define BMJ_DSPTFL (-1875.f * BMJ_FR)
#define BMJ_DSPBFS (-3875.f)
#define BMJ_DSP0FS (-5875.f)
#define BMJ_DSPTFS (-1875.f)
#define BMJ_PL 2500.f
#define BMJ_PLQ 70000.f
#define BMJ_PH 105000.f
#define BMJ_THL 210.f
#define BMJ_THH 365.f
#define BMJ_THHQ 325.f
#define BMJ_RDP ((BMJ_ITB - 1.f) / (BMJ_PH - BMJ_PL))
#define BMJ_RDPQ ((BMJ_ITBQ - 1.f) / (BMJ_PH - BMJ_PLQ))
#define BMJ_RDQ ((float)(BMJ_ITB - 1))
#define BMJ_RDTH ((BMJ_JTB - 1.f) / (BMJ_THH - BMJ_THL))
#define BMJ_RDTHE (BMJ_JTB - 1.f)
#define BMJ_RDTHEQ (BMJ_JTBQ - 1.f)
#define BMJ_RSFCP (1.f / 101300.f)
#define BMJ_AVGEFI ((BMJ_EFIMN + 1.f) * 0.5f)
#define BMJ_DSPBSL (BMJ_DSPBFL * BMJ_FSL)
#define BMJ_DSP0SL (BMJ_DSP0FL * BMJ_FSL)
#define BMJ_DSPTSL (BMJ_DSPTFL * BMJ_FSL)
#define BMJ_DSPBSS (BMJ_DSPBFS * BMJ_FSS)
#define BMJ_DSP0SS (BMJ_DSP0FS * BMJ_FSS)
#define BMJ_DSPTSS (BMJ_DSPTFS * BMJ_FSS)
#define BMJ_ELEVFC 0.6f
#define BMJ_STEFI 1.f
#define BMJ_SLOPBL ((BMJ_DSPBFL - BMJ_DSPBSL) / (1.f - BMJ_EFIMN))
#define BMJ_SLOP0L ((BMJ_DSP0FL - BMJ_DSP0SL) / (1.f - BMJ_EFIMN))
#define BMJ_SLOPTL ((BMJ_DSPTFL - BMJ_DSPTSL) / (1.f - BMJ_EFIMN))
#define BMJ_SLOPBS ((BMJ_DSPBFS - BMJ_DSPBSS) / (1.f - BMJ_EFIMN))
#define BMJ_SLOP0S ((BMJ_DSP0FS - BMJ_DSP0SS) / (1.f - BMJ_EFIMN))
#define BMJ_SLOPTS ((BMJ_DSPTFS - BMJ_DSPTSS) / (1.f - BMJ_EFIMN))
#define BMJ_SLOPST ((BMJ_STABDF - BMJ_STABDS) / (1.f - BMJ_EFIMN))
#define BMJ_SLOPE ((1.f - BMJ_EFMNT) / (1.f - BMJ_EFIMN))
#define BMJ_A2 17.2693882f
#define BMJ_A3 273.16f
#define BMJ_A4 35.86f
#define BMJ_PQ0 379.90516f
#define BMJ_EPSQ 1.e-12f
/* what cu_driver.f90:448-449 passes: cp (icar_constants), r_d, xlv (mod_wrf_constants), gravity, svpt0, EP1 = Rw/Rd - 1 (icar_constants) */
#define BMJ_CP 1012.0f
#define BMJ_R 287.f
#define BMJ_ELWV 2.5E6f
#define BMJ_G 9.81f
#define BMJ_TFRZ 273.15f
#define BMJ_D608 (461.5f / 287.058f - 1.f)
#define BMJ_CAPA (BMJ_R / BMJ_CP)
#define BMJ_CPRLG (BMJ_CP / (BMJ_ROW * BMJ_G * BMJ_ELWV))
#define BMJ_ELOCP (BMJ_ELIWV / BMJ_CP)
#define BMJ_RCP (1.f / BMJ_CP)
#define BMJ_A23M4L (BMJ_A2 * (BMJ_A3 - BMJ_A4) * BMJ_ELWV)

#define BMJ_WS(a, L) ws[((size_t)(a) * nl + (size_t)((L) - 1)) * stride]
#define BMJ_AINT(x) __builtin_truncf(x)

/* TTBLEX :1743-1819: the temperature of the moist adiabat THESP at the pressure prsmid, from the coarse table below PLQ, else the fine */
BMJ_FN float bmj_ttblex(const BmjTables *tb, float prsmid, float thesp)
{
    const int fine = !(prsmid < BMJ_PLQ);                              /* :785, :817, :974 */
    const int itbx = fine ? BMJ_ITBQ : BMJ_ITB, jtbx = fine ? BMJ_JTBQ : BMJ_JTB;
    const float plx = fine ? BMJ_PLQ : BMJ_PL, rdpx = fine ? BMJ_RDPQ : BMJ_RDP, rdthex = fine ? BMJ_RDTHEQ : BMJ_RDTHE;
    const float *sthe = fine ? tb->STHEQ : tb->STHE, *the0 = fine ? tb->THE0Q : tb->THE0, *ttbl = fine ? tb->TTBLQ : tb->TTBL;
    const float tpk = (prsmid - plx) * rdpx;
    float qq = tpk - BMJ_AINT(tpk);
    int iptb = (int)tpk + 1;
    if (iptb < 1) { iptb = 1; qq = 0.f; }
    if (iptb >= itbx) { iptb = itbx - 1; qq = 0.f; }
    const float bthe00k = the0[iptb - 1], sthe00k = sthe[iptb - 1], bthe10k = the0[iptb], sthe10k = sthe[iptb];
    const float bthk = (bthe10k - bthe00k) * qq + bthe00k, sthk = (sthe10k - sthe00k) * qq + sthe00k;
    const float tthk = (thesp - bthk) / sthk * rdthex;
    float pp = tthk - BMJ_AINT(tthk);
    int ithtb = (int)tthk + 1;
    if (ithtb < 1) { ithtb = 1; pp = 0.f; }
    if (ithtb >= jtbx) { ithtb = jtbx - 1; pp = 0.f; }
    const float *c0 = ttbl + (size_t)jtbx * (iptb - 1) + (ithtb - 1), *c1 = c0 + jtbx;
    const float t00k = c0[0], t10k = c0[1], t01k = c1[0], t11k = c1[1];
    return (t00k + (t10k - t00k) * pp + (t01k - t00k) * qq + (t00k - t10k - t01k + t11k) * pp * qq);
}

/* the saturation-point pressure of (theta, q) from PTBL: :564-607 and :1472-1522 share the index arithmetic */
BMJ_FN void bmj_ptbl_index(const BmjTables *tb, float th, float q, int *it_, int *iq_, float *qq_, float *pp_)
{
    const float tth = (th - BMJ_THL) * BMJ_RDTH;
    float qq = tth - BMJ_AINT(tth);
    int it = (int)tth + 1;
    if (it < 1) { it = 1; qq = 0.f; }
    else if (it >= BMJ_JTB) { it = BMJ_JTB - 1; qq = 0.f; }
    const float bqs00k = tb->QS0[it - 1], sqs00k = tb->SQS[it - 1], bqs10k = tb->QS0[it], sqs10k = tb->SQS[it];
    const float bq = (bqs10k - bqs00k) * qq + bqs00k, sq = (sqs10k - sqs00k) * qq + sqs00k;
    const float tq = (q - bq) / sq * BMJ_RDQ;
    float pp = tq - BMJ_AINT(tq);
    int iq = (int)tq + 1;
    if (iq < 1) { iq = 1; pp = 0.f; }
    else if (iq >= BMJ_ITB) { iq = BMJ_ITB - 1; pp = 0.f; }
    *it_ = it; *iq_ = iq; *qq_ = qq; *pp_ = pp;
}

BMJ_FN float bmj_qsat(float p, float t) { return BMJ_PQ0 / p * BMJ_EXPF(BMJ_A2 * (t - BMJ_A3) / (t - BMJ_A4)); }
/* (tup (qfac) - t (q 0.608 + 1)) 0.5 / (t (q 0.608 + 1)) of :743-745 and its kin */
BMJ_FN float bmj_trm(float tup, float fac, float t, float q) { const float tv = t * (q * 0.608f + 1.f); return (tup * fac - tv) * 0.5f / tv; }

typedef struct BmjOut { int lbot, ltop, kind; float pcpcol, cldefi; } BmjOut;
/* what the buoyancy search hands to the adjustment: the parcel of maximum CAPE (PSPcnv, THBTcnv, THESP of THEScnv, LBOTcnv, LTOPcnv),
 * which of the two (CPE, DTV) pairs holds CPEcnv / DTVcnv, and whether any parcel had CAPE */
typedef struct BmjSearch { float psp, thbt, thesp; int lbot, ltop, pair, found; } BmjSearch;

#define T_(L) BMJ_WS(BMJ_T, L)
#define Q_(L) BMJ_WS(BMJ_Q, L)
#define P_(L) BMJ_WS(BMJ_P, L)
#define DPRS_(L) BMJ_WS(BMJ_DP, L)
#define APE_(L) BMJ_WS(BMJ_APE, L)
#define TREFK_(L) BMJ_WS(BMJ_TREFK, L)
#define QREFK_(L) BMJ_WS(BMJ_QREFK, L)
#define CPE_(L) BMJ_WS(cur ? BMJ_CPE1 : BMJ_CPE0, L)
#define DTV_(L) BMJ_WS(cur ? BMJ_DTV1 : BMJ_DTV0, L)

/* BMJ :496-882 on the levels 1..lmh of the workspace (T, Q, P filled by the caller): APE and the search for the level of maximum
 * buoyancy.  Touches T, Q, P, APE and the two (CPE, DTV) pairs only. */
BMJ_FN BmjSearch bmj_search(float *ws, size_t stride, int nl, int lmh, const BmjTables *tb)
{
    int lbot = lmh, ltop = lmh, L;
    float psp = 0.f, thbt = 0.f, pbot = 0.f, ptop = 0.f;

    for (L = 1; L <= lmh; ++L) APE_(L) = BMJ_POWF(1.E5f / P_(L), BMJ_CAPA);                           /* :523-529 */

    /* ---- the search for the level of maximum buoyancy, :535-882 ---- */
    const float plmh = P_(lmh), pelevfc = plmh * BMJ_ELEVFC, pbtmx = P_(lmh) - BMJ_PONE;
    float capecnv = 0.f, pspcnv = 0.f, thbtcnv = 0.f, thespcnv = 0.f, thesp = 0.f;
    int lbotcnv = lbot, ltopcnv = lbot;
    int cur = 0;                                  /* which of the two (CPE, DTV) pairs the trial parcel writes; the other holds CPEcnv, DTVcnv */
    for (int kb = lmh; kb >= 1; --kb) {
        const float pkl = P_(kb);
        if (pkl < pelevfc) break;                                                                      /* :554 */
        lbot = lmh; ltop = lmh;
        const float qbt = Q_(kb);
        thbt = T_(kb) * APE_(kb);
        int it, iq; float qq1, pp1;
        bmj_ptbl_index(tb, thbt, qbt, &it, &iq, &qq1, &pp1);
        {
            const float *r0 = tb->PTBL + (size_t)BMJ_ITB * (it - 1) + (iq - 1), *r1 = r0 + BMJ_ITB;
            const float p00k = r0[0], p10k = r0[1], p01k = r1[0], p11k = r1[1];
            psp = p00k + (p10k - p00k) * pp1 + (p01k - p00k) * qq1 + (p00k - p10k - p01k + p11k) * pp1 * qq1;   /* :606 */
        }
        const float apes = BMJ_POWF(1.E5f / psp, BMJ_CAPA);
        thesp = thbt * BMJ_EXPF(BMJ_ELOCP * qbt * apes / thbt);                                       /* :609 */
        for (L = 1; L <= lmh - 1; ++L) { const float p = P_(L); if (p < psp && p >= BMJ_PQM) lbot = L + 1; }   /* :615-618 */
        pbot = P_(lbot);
        if (pbot >= pbtmx || lbot >= lmh) {                                                            /* :624-630 */
            for (L = 1; L <= lmh - 1; ++L) if (P_(L) < pbtmx) lbot = L;
            pbot = P_(lbot);
        }
        ltop = lbot; ptop = pbot;
        if (lbot >= lmh) continue;                /* the reference reads level lmh+1 from here on (header) */
        for (L = 1; L <= lmh; ++L) { CPE_(L) = 0.f; DTV_(L) = 0.f; }                                   /* :721-724 */
        float dentpy = 0.f, plo = P_(kb), trmlo = 0.f, pup, tup, dp, trmup;
        const float capetrigr = BMJ_DTPTRIGR / T_(lbot);
        const float facbt = qbt * 0.608f + 1.f;
        int stop = 0;
        if (kb > lbot) {                                                                               /* :738-752 below cloud base */
            for (L = kb - 1; L >= lbot + 1; --L) {
                pup = P_(L); tup = thbt / APE_(L); dp = plo - pup;
                trmup = bmj_trm(tup, facbt, T_(L), Q_(L));
                const float dtv = trmlo + trmup;
                DTV_(L) = dtv;
                dentpy = dtv * dp + dentpy;
                CPE_(L) = dentpy;
                if (dentpy < capetrigr) { stop = 1; break; }
                plo = pup; trmlo = trmup;
            }
        } else {                                                                                       /* :753-760 */
            L = lbot + 1;
            plo = P_(L); tup = thbt / APE_(L);
            trmlo = bmj_trm(tup, facbt, T_(L), Q_(L));
        }
        if (!stop) {                                                                                   /* :764-806 at cloud base */
            L = lbot;
            pup = psp; tup = thbt / apes;
            const float tsp = (T_(L + 1) - T_(L)) / (plo - pbot) * (pup - pbot) + T_(L);
            const float qsp = (Q_(L + 1) - Q_(L)) / (plo - pbot) * (pup - pbot) + Q_(L);
            dp = plo - pup;
            trmup = bmj_trm(tup, facbt, tsp, qsp);
            float dtv = trmlo + trmup;
            dentpy = dtv * dp + dentpy;
            dtv = dtv * dp;
            plo = pup; trmlo = trmup;
            pup = P_(L);
            tup = bmj_ttblex(tb, pup, thesp);
            float qup = bmj_qsat(pup, tup), qwat = qbt - qup;
            dp = plo - pup;
            trmup = bmj_trm(tup, qup * 0.608f + 1.f - qwat, T_(L), Q_(L));
            dentpy = (trmlo + trmup) * dp + dentpy;
            CPE_(L) = dentpy;
            DTV_(L) = (dtv + (trmlo + trmup) * dp) / (P_(lbot + 1) - P_(lbot));
            if (dentpy < capetrigr) stop = 1;
            else {
                plo = pup; trmlo = trmup;
                for (L = lbot - 1; L >= 1; --L) {                                                      /* :812-839 in cloud */
                    pup = P_(L);
                    tup = bmj_ttblex(tb, pup, thesp);
                    qup = bmj_qsat(pup, tup); qwat = qbt - qup;
                    dp = plo - pup;
                    trmup = bmj_trm(tup, qup * 0.608f + 1.f - qwat, T_(L), Q_(L));
                    dtv = trmlo + trmup;
                    DTV_(L) = dtv;
                    dentpy = dtv * dp + dentpy;
                    CPE_(L) = dentpy;
                    if (dentpy < capetrigr) break;
                    plo = pup; trmlo = trmup;
                }
            }
        }
        int ltp1 = kb;                                                                                 /* 170, :843-860 */
        float cape = 0.f;
        for (L = kb; L >= 1; --L) {
            const float c = CPE_(L);
            if (c < capetrigr) break;
            else if (c > cape) { ltp1 = L; cape = c; }
        }
        ltop = ltp1 < lbot ? ltp1 : lbot;
        if (cape > capecnv) {                                                                          /* :865-876 */
            capecnv = cape; pspcnv = psp; thbtcnv = thbt; lbotcnv = lbot; ltopcnv = ltop; thespcnv = thesp;
            cur ^= 1;                             /* this parcel's CPE / DTV become CPEcnv / DTVcnv */
        }
    }
    (void)ptop;
    {
        BmjSearch r;
        r.psp = pspcnv; r.thbt = thbtcnv; r.thesp = thespcnv; r.lbot = lbotcnv; r.ltop = ltopcnv; r.pair = cur ^ 1; r.found = capecnv > 0.f;
        return r;
    }
}

/* BMJ :888-1739: the quick exit, deep and shallow convection for the parcel the search found.  kind != BMJ_NONE: DTDT / DQDT of the
 * levels ltop..lbot are in BMJ_DIFT / BMJ_DIFQ, zero elsewhere (not stored). */
BMJ_FN BmjOut bmj_adjust(float *ws, size_t stride, int nl, int lmh, float dtcnvc, float sm, float cldefi, float psfc, const BmjTables *tb, BmjSearch f)
{
    const int kte = lmh, cur = f.pair;            /* CPE_, DTV_ read CPEcnv, DTVcnv (:896-900) */
    BmjOut out;
    const float rdtcnvc = 1.f / dtcnvc;
    const float depmin = BMJ_PSH * psfc * BMJ_RSFCP;
    const float tauk = dtcnvc / BMJ_TREL, tauksc = dtcnvc / (1.0f * BMJ_TREL);
    int lbot = f.lbot, ltop = f.ltop, shallow = 0, L;
    const float psp = f.psp, thbt = f.thbt, thesp = f.thesp;
    float pbot = 0.f, ptop = 0.f;
    out.pcpcol = 0.f; out.kind = BMJ_NONE;
    if (f.found) { pbot = P_(lbot); ptop = P_(ltop); }                                                 /* :888-902 */
    if (!f.found || ptop > pbot - BMJ_PNO || ltop > lbot - 2) {                                        /* :908-916 */
        out.lbot = 0; out.ltop = kte;
        out.cldefi = BMJ_AVGEFI * sm + BMJ_STEFI * (1.f - sm);
        return out;
    }
    float depth = pbot - ptop;
    if (depth >= depmin) {
        /* ---- deep convection, :939-1334 ---- */
        const int lb = lbot;
        float efi = cldefi;
        for (L = ltop > 1 ? ltop - 1 : 1; L <= lb; ++L) BMJ_WS(BMJ_THERK, L) = bmj_ttblex(tb, P_(L), thesp) * APE_(L);   /* :974-981 */
        const int lbm1 = lb - 1;
        const float pkb = P_(lb), pkt = P_(ltop);
        const float stabdl = (efi - BMJ_EFIMN) * BMJ_SLOPST + BMJ_STABDS;
        int l0 = lb, frozen = 0;
        float pk0 = P_(lb), trefkx = T_(lb), therkx = BMJ_WS(BMJ_THERK, lb), apekxx = APE_(lb), therky = BMJ_WS(BMJ_THERK, lbm1), apekxy = APE_(lbm1);
        TREFK_(lb) = trefkx;
        for (L = lbm1; L >= ltop; --L) {                                                               /* :1003-1015 */
            if (T_(L + 1) < BMJ_TFRZ) { frozen = 1; break; }
            trefkx = ((therky - therkx) * stabdl + trefkx * apekxx) / apekxy;
            TREFK_(L) = trefkx;
            apekxx = apekxy; therkx = therky;
            if (L > 1) { apekxy = APE_(L - 1); therky = BMJ_WS(BMJ_THERK, L - 1); }
            l0 = L; pk0 = P_(l0);
        }
        if (frozen) {                                                                                  /* 430, :1023-1030 */
            const float rdp0t = 1.f / (pk0 - pkt);
            const float dthem = BMJ_WS(BMJ_THERK, l0) - TREFK_(l0) * APE_(l0);
            for (L = ltop; L <= l0 - 1; ++L) TREFK_(L) = (BMJ_WS(BMJ_THERK, L) - (P_(L) - pkt) * dthem * rdp0t) / APE_(L);
        }
        const float depwl = pkb - pk0;                                                                 /* 450 */
        depth = BMJ_PFRZ * psfc * BMJ_RSFCP;
        const float sm1 = 1.f - sm, pbotfc = 1.f;
        float dentpy = 0.f, preck = 0.f, pdqd = 0.f, prwd = 0.f, sumdp = 0.f;
        for (int itrefi = 1; itrefi <= 3; ++itrefi) {                                                  /* :1065-1200 */
            const float dspbk = ((efi - BMJ_EFIMN) * BMJ_SLOPBS + BMJ_DSPBSS * pbotfc) * sm + ((efi - BMJ_EFIMN) * BMJ_SLOPBL + BMJ_DSPBSL * pbotfc) * sm1;
            const float dsp0k = ((efi - BMJ_EFIMN) * BMJ_SLOP0S + BMJ_DSP0SS * pbotfc) * sm + ((efi - BMJ_EFIMN) * BMJ_SLOP0L + BMJ_DSP0SL * pbotfc) * sm1;
            const float dsptk = ((efi - BMJ_EFIMN) * BMJ_SLOPTS + BMJ_DSPTSS * pbotfc) * sm + ((efi - BMJ_EFIMN) * BMJ_SLOPTL + BMJ_DSPTSL * pbotfc) * sm1;
            for (L = ltop; L <= lb; ++L) {                                                             /* :1077-1108 */
                const float pk = P_(L);
                float dsp;
                if (depwl >= depth) {
                    if (L < l0) dsp = ((pk0 - pk) * dsptk + (pk - pkt) * dsp0k) / (pk0 - pkt);
                    else        dsp = ((pkb - pk) * dsp0k + (pk - pk0) * dspbk) / (pkb - pk0);
                } else {
                    dsp = dsp0k;
                    if (L < l0) dsp = ((pk0 - pk) * dsptk + (pk - pkt) * dsp0k) / (pk0 - pkt);
                }
                const float psk = pk + dsp, apesk = BMJ_POWF(1.E5f / psk, BMJ_CAPA);
                BMJ_WS(BMJ_PSK, L) = psk; BMJ_WS(BMJ_APESK, L) = apesk;
                if (pk > BMJ_PQM) {
                    const float thsk = TREFK_(L) * APE_(L);
                    QREFK_(L) = BMJ_PQ0 / psk * BMJ_EXPF(BMJ_A2 * (thsk - BMJ_A3 * apesk) / (thsk - BMJ_A4 * apesk));
                } else QREFK_(L) = Q_(L);
            }
            for (int iter = 1; iter <= 2; ++iter) {                                                    /* :1114-1157 */
                float sumde = 0.f, dhdt = 0.f;
                sumdp = 0.f;
                for (L = ltop; L <= lb; ++L) {
                    const float dprs = DPRS_(L), trefk = TREFK_(L), qrefk = QREFK_(L);
                    sumde = ((T_(L) - trefk) * BMJ_CP + (Q_(L) - qrefk) * BMJ_ELWV) * dprs + sumde;
                    const float x = (trefk * APE_(L) / BMJ_WS(BMJ_APESK, L)) - BMJ_A4;
                    dhdt = (qrefk * BMJ_A23M4L / (x * x) + BMJ_CP) * dprs + dhdt;
                    sumdp = sumdp + dprs;
                }
                const float hcorr = sumde / (sumdp - DPRS_(ltop));
                dhdt = dhdt / (sumdp - DPRS_(ltop));
                int lcor = ltop + 1, lqm = 1;
                for (L = 1; L <= lb; ++L) if (P_(L) <= BMJ_PQM) lqm = L;
                if (lcor <= lqm) {
                    for (L = lcor; L <= lqm; ++L) TREFK_(L) = TREFK_(L) + hcorr * BMJ_RCP;
                    lcor = lqm + 1;
                }
                for (L = lcor; L <= lb; ++L) {
                    const float trefk = hcorr / dhdt + TREFK_(L);
                    TREFK_(L) = trefk;
                    const float thskl = trefk * APE_(L), apesk = BMJ_WS(BMJ_APESK, L);
                    QREFK_(L) = BMJ_PQ0 / BMJ_WS(BMJ_PSK, L) * BMJ_EXPF(BMJ_A2 * (thskl - BMJ_A3 * apesk) / (thskl - BMJ_A4 * apesk));
                }
            }
            float avrgt = 0.f, dsq = 0.f, dst = 0.f;                                                   /* :1163-1197 */
            preck = 0.f; pdqd = 0.f; prwd = 0.f;
            for (L = ltop; L <= lb; ++L) {
                const float tkl = T_(L), qk = Q_(L), qrefk = QREFK_(L), dprs = DPRS_(L);
                const float diftl = (TREFK_(L) - tkl) * tauk;
                const float difql = (qrefk - qk) * tauk;
                const float avrgtl = (tkl + tkl + diftl);
                const float dpot = dprs / avrgtl;
                dst = diftl * dpot + dst;
                dsq = difql * BMJ_ELWV * dpot + dsq;
                avrgt = avrgtl * dprs + avrgt;
                preck = diftl * dprs + preck;
                pdqd = (qk - qrefk) * dprs + pdqd;
                prwd = qk * dprs + prwd;
                BMJ_WS(BMJ_DIFT, L) = diftl;
                BMJ_WS(BMJ_DIFQ, L) = difql;
            }
            dst = (dst + dst) * BMJ_CP;
            dsq = dsq + dsq;
            dentpy = dst + dsq;
            avrgt = avrgt / (sumdp + sumdp);
            const float pk7 = 1.E-7f > preck ? 1.E-7f : preck;
            float drheat = (preck * sm + pk7 * (1.f - sm)) * BMJ_CP / avrgt;
            drheat = drheat > 1.E-20f ? drheat : 1.E-20f;
            efi = BMJ_EFIFC * dentpy / drheat;
            efi = efi < 1.f ? efi : 1.f;
            efi = efi > BMJ_EFIMN ? efi : BMJ_EFIMN;
        }
        (void)pdqd; (void)prwd;                   /* DQCOL, PWCOL: the radiation feedback block alone reads them (not built) */
        if (dentpy >= BMJ_EPSNTP && preck > BMJ_EPSPR) {                                               /* :1208-1226 */
            float fefi = BMJ_EFMNT + BMJ_SLOPE * (efi - BMJ_EFIMN);
            fefi = (dentpy - BMJ_EPSNTP) * fefi / dentpy;
            preck = preck * fefi;
            out.pcpcol = preck * BMJ_CPRLG;
            for (L = ltop; L <= lb; ++L) {
                BMJ_WS(BMJ_DIFT, L) = BMJ_WS(BMJ_DIFT, L) * fefi * rdtcnvc;
                BMJ_WS(BMJ_DIFQ, L) = BMJ_WS(BMJ_DIFQ, L) * fefi * rdtcnvc;
            }
            out.cldefi = efi; out.lbot = lbot; out.ltop = ltop; out.kind = BMJ_DEEP;
            return out;
        }
        cldefi = BMJ_EFIMN * sm + BMJ_STEFI * (1.f - sm);                                              /* :1246 */
        float ptpk = P_(lbot) - depmin;                                                                /* :1256-1262 */
        ptpk = BMJ_PSHU > ptpk ? BMJ_PSHU : ptpk;
        for (L = 1; L <= lmh; ++L) if (P_(L) <= ptpk) ltop = L + 1;
        int ltp1 = lbot;                                                                               /* :1314-1322 */
        for (L = lbot - 1; L >= ltop; --L) { if (DTV_(L) > 0.f) ltp1 = L; else break; }
        ltop = ltp1 < lbot ? ltp1 : lbot;
        ptop = P_(ltop);
        shallow = 1;
    } else shallow = 1;                                                                                /* :926-928 */
    out.cldefi = cldefi;
    out.lbot = 0; out.ltop = kte;                 /* every refusal below leaves these (:1463-1467 and the like) */
    if (!shallow) return out;

    /* ---- shallow convection, :1380-1719 ---- */
    {
        const float pkb_ = P_(lbot), tb_ = T_(lbot);
        const float tlev2 = tb_ * BMJ_POWF((pkb_ - BMJ_PONE) / pkb_, BMJ_CAPA);                       /* :1407-1410 */
        const float qsat1 = bmj_qsat(pkb_, tb_);
        const float qsat2 = BMJ_PQ0 / (pkb_ - BMJ_PONE) * BMJ_EXPF(BMJ_A2 * (tlev2 - BMJ_A3) / (tlev2 - BMJ_A4));
        const float rhshmax = qsat2 / qsat1;
        float sumdp = 0.f, rhavg = 0.f;
        for (L = lbot; L >= ltop; --L) {                                                               /* :1414-1417 */
            rhavg = rhavg + DPRS_(L) * Q_(L) / bmj_qsat(P_(L), T_(L));
            sumdp = sumdp + DPRS_(L);
        }
        if (rhavg / sumdp > rhshmax) {                                                                 /* :1419-1433 */
            int ltsh = ltop;
            for (L = ltop - 1; L >= 1; --L) {
                rhavg = rhavg + DPRS_(L) * Q_(L) / bmj_qsat(P_(L), T_(L));
                sumdp = sumdp + DPRS_(L);
                if (CPE_(L) > 0.f) ltsh = L; else break;
                if (rhavg / sumdp <= rhshmax) break;
                if (P_(L) <= BMJ_PSHU) break;
            }
            ltop = ltsh;
        }
    }
    if (ltop < 2) ltop = 2;                                                                            /* :1439-1443 */
    const int ltp1 = ltop - 1;
    if (ptop > pbot - BMJ_PNO || ltop > lbot - 2) return out;                                          /* :1462-1468 (PTOP is not that of a raised top) */
    const float thtpk = T_(ltp1) * APE_(ltp1);                                                         /* :1472 */
    float ptpk;
    {
        int it, iq; float qqk, ppk;
        bmj_ptbl_index(tb, thtpk, Q_(ltp1), &it, &iq, &qqk, &ppk);
        const float *r0 = tb->PTBL + (size_t)BMJ_ITB * (it - 1) + (iq - 1), *r1 = r0 + BMJ_ITB;
        const float part1 = (r0[1] - r0[0]) * ppk, part2 = (r1[0] - r0[0]) * qqk;
        const float part3 = (r0[0] - r0[1] - r1[0] + r1[1]) * ppk * qqk;
        ptpk = r0[0] + part1 + part2 + part3;                                                          /* :1518-1522 */
    }
    float dpmix = ptpk - psp;
    if (__builtin_fabsf(dpmix) < 3000.f) dpmix = -3000.f;
    const float smix = (thtpk - thbt) / dpmix * BMJ_STABS;                                             /* :1529 */
    {
        float trefkx = T_(lbot + 1), pkxxxx = P_(lbot + 1), pkxxxy = P_(lbot), apekxx = APE_(lbot + 1), apekxy = APE_(lbot);
        const int lmid = (int)(.5f * (float)(lbot + ltop));
        for (L = lbot; L >= ltop; --L) {                                                               /* :1539-1548 */
            trefkx = ((pkxxxy - pkxxxx) * smix + trefkx * apekxx) / apekxy;
            float tr = trefkx;
            if (L <= lmid) { const float lo = T_(L) + BMJ_DTSHAL; tr = tr > lo ? tr : lo; }
            TREFK_(L) = tr;
            apekxx = apekxy; pkxxxx = pkxxxy;
            apekxy = APE_(L - 1); pkxxxy = P_(L - 1);                  /* ltop >= 2 */
        }
    }
    float sumdt = 0.f, sumdp = 0.f;                                                                    /* :1552-1569 */
    for (L = ltop; L <= lbot; ++L) { sumdt = (T_(L) - TREFK_(L)) * DPRS_(L) + sumdt; sumdp = sumdp + DPRS_(L); }
    const float rdpsum = 1.f / sumdp, tcorr = sumdt * rdpsum;
    for (L = ltop; L <= lbot; ++L) TREFK_(L) = TREFK_(L) + tcorr;
    float psum = 0.f, qsum = 0.f, potsum = 0.f, qotsum = 0.f, otsum = 0.f, dst = 0.f;                  /* :1573-1597 */
    const float fptk = TREFK_(ltop);
    for (L = ltop; L <= lbot; ++L) {
        const float trefk = TREFK_(L), tk = T_(L), qk = Q_(L), dprs = DPRS_(L);
        const float dpkl = trefk - fptk;
        psum = dpkl * dprs + psum;
        qsum = qk * dprs + qsum;
        const float rtbar = 2.f / (trefk + tk);
        otsum = dprs * rtbar + otsum;
        potsum = dpkl * rtbar * dprs + potsum;
        qotsum = qk * rtbar * dprs + qotsum;
        dst = (trefk - tk) * rtbar * dprs / BMJ_ELWV + dst;
    }
    psum = psum * rdpsum; qsum = qsum * rdpsum;
    const float rotsum = 1.f / otsum;
    potsum = potsum * rotsum; qotsum = qotsum * rotsum;
    dst = dst * rotsum * BMJ_CP;
    if (dst > 0.f) return out;                                                                         /* :1610-1619 */
    const float dstq = dst * BMJ_EPSDN;
    const float den = potsum - psum;
    if (-den / psum < 5.E-5f) return out;                                                              /* :1625-1636 */
    const float dqref = (qotsum - dstq - qsum) / den;
    if (dqref < 0.f) return out;                                                                       /* :1640-1646 */
    const float qrftp = qsum - dqref * psum;
    for (L = ltop; L <= lbot; ++L) {                                                                   /* :1654-1684 */
        const float trefk = TREFK_(L), tk = T_(L), qk = Q_(L);
        const float qrfkl = (trefk - fptk) * dqref + qrftp;
        const float tnew = (trefk - tk) * tauksc + tk;
        const float qsatk = bmj_qsat(P_(L), tnew);
        const float qnew = (qrfkl - qk) * tauksc + qk;
        if (qnew < qsatk * BMJ_RHLSC) return out;
        if (qnew > qsatk * BMJ_RHHSC) return out;
        BMJ_WS(BMJ_THVREF, L) = trefk * APE_(L) * (qrfkl * BMJ_D608 + 1.f);
        QREFK_(L) = qrfkl;
    }
    for (L = ltop; L <= lbot; ++L) {                                                                   /* :1700-1711 */
        const float above = L == ltop ? T_(L - 1) * APE_(L - 1) * (Q_(L - 1) * BMJ_D608 + 1.f) : BMJ_WS(BMJ_THVREF, L - 1);   /* THVREF(LTOP-1): :1392-1393 */
        const float dtdp = (above - BMJ_WS(BMJ_THVREF, L)) / (P_(L) - P_(L - 1));
        if (dtdp < BMJ_EPSDT) return out;
    }
    for (L = ltop; L <= lbot; ++L) {                                                                   /* :1716-1719 */
        BMJ_WS(BMJ_DIFT, L) = (TREFK_(L) - T_(L)) * tauksc * rdtcnvc;
        BMJ_WS(BMJ_DIFQ, L) = (QREFK_(L) - Q_(L)) * tauksc * rdtcnvc;
    }
    out.lbot = lbot; out.ltop = ltop; out.kind = BMJ_SHALLOW;
    return out;
}

/* BMJ :393-1739 */
BMJ_FN BmjOut bmj_column(float *ws, size_t stride, int nl, int lmh, float dtcnvc, float sm, float cldefi, float psfc, const BmjTables *tb)
{
    return bmj_adjust(ws, stride, nl, lmh, dtcnvc, sm, cldefi, psfc, tb, bmj_search(ws, stride, nl, lmh, tb));
}

/* The fields of one column, each pointing at (i, kts, j); consecutive levels lie `sk` floats apart. */
typedef struct BmjCol { const float *t, *qv, *pmid, *pint, *pi, *rho, *dz; float *tend_th, *tend_qv; } BmjCol;

/* BMJDRV :175-265 for one column with n = kte-1 - kts + 1 levels (STEPCU = 1, LOWLYR = 1; kts = 1, see cu_bmj.hip), in three parts
 * (the middle one in two: bmj_search, bmj_col_adjust) that the device runs as kernels of their own -- the scheme's control flow then
 * carries none of the fields' pointers -- and the host one after the other.
 * xland: cu_driver.f90:139-140.  tend_th / tend_qv of the n levels, raincv, cutop, cubot and cldefi are written. */
BMJ_FN void bmj_col_load(BmjCol c, size_t sk, int n, float *ws, size_t stride)                         /* :206-216 */
{
    const int nl = n;
    for (int k = 1; k <= n; ++k) {
        const size_t o = (size_t)(n - k) * sk;    /* KFLIP - 1 */
        const float qv = c.qv[o], q = qv / (1.f + qv);
        BMJ_WS(BMJ_Q, k) = BMJ_EPSQ > q ? BMJ_EPSQ : q;
        BMJ_WS(BMJ_T, k) = c.t[o];
        BMJ_WS(BMJ_P, k) = c.pmid[o];
        BMJ_WS(BMJ_DP, k) = c.rho[o] * BMJ_G * c.dz[o];
    }
}

BMJ_FN int bmj_col_adjust(int n, float dt, float xland, float psfc, float *cldefi, float *raincv, float *cutop, float *cubot, float *ws,
                          size_t stride, const BmjTables *tb, BmjSearch f)
{
    const float dtcnvc = dt * 1.f;                                                                     /* :173 */
    const float landmask = xland - 1.f;                                                                /* :200 */
    const BmjOut r = bmj_adjust(ws, stride, n, n, dtcnvc, landmask, *cldefi, psfc, tb, f);
    *raincv = r.pcpcol * 1.E3f / 1.f;                                                                  /* :259 */
    *cutop = (float)(n + 1 - r.ltop);                                                                  /* :264-265 */
    *cubot = (float)(n + 1 - r.lbot);
    *cldefi = r.cldefi;
    return r.kind;
}

BMJ_FN int bmj_col_run(int n, float dt, float xland, float psfc, float *cldefi, float *raincv, float *cutop, float *cubot, float *ws, size_t stride,
                       const BmjTables *tb)
{
    return bmj_col_adjust(n, dt, xland, psfc, cldefi, raincv, cutop, cubot, ws, stride, tb, bmj_search(ws, stride, n, n, tb));
}

/* cutop, cubot: what bmj_col_run left (LBOT = 0, so CUBOT = n + 1, says that DTDT and DQDT are zero) */
BMJ_FN void bmj_col_store(BmjCol c, size_t sk, int n, float cutop, float cubot, const float *ws, size_t stride)   /* :246-253 */
{
    const int nl = n, ltop = n + 1 - (int)cutop, lbot = n + 1 - (int)cubot;
    for (int k = 1; k <= n; ++k) {
        const int kflip = n + 1 - k;
        const size_t o = (size_t)(k - 1) * sk;
        const int in = lbot != 0 && kflip >= ltop && kflip <= lbot;
        const float dtdt = in ? BMJ_WS(BMJ_DIFT, kflip) : 0.f, dqdt = in ? BMJ_WS(BMJ_DIFQ, kflip) : 0.f;
        const float om = 1.f - BMJ_WS(BMJ_Q, kflip);
        c.tend_th[o] = dtdt / c.pi[o];
        c.tend_qv[o] = dqdt / (om * om);
    }
}

BMJ_FN int bmj_drv_column(BmjCol c, size_t sk, int n, float dt, float xland, float *cldefi, float *raincv, float *cutop, float *cubot,
                          float *ws, size_t stride, const BmjTables *tb)
{
    bmj_col_load(c, sk, n, ws, stride);
    const int kind = bmj_col_run(n, dt, xland, c.pint[0], cldefi, raincv, cutop, cubot, ws, stride, tb);   /* PSFC :195 */
    bmj_col_store(c, sk, n, *cutop, *cubot, ws, stride);
    return kind;
}

#ifdef BMJ_WITH_TABLES
/* host only; BMJ_HOST_EXPF / BMJ_HOST_POWF: the C library's, where BMJ_EXPF / BMJ_POWF name device functions */
#ifndef BMJ_HOST_EXPF
#define BMJ_HOST_EXPF BMJ_EXPF
#define BMJ_HOST_POWF BMJ_POWF
#endif
/* SPLINE :2090-2198; every array 1-based */
static void bmj_spline(int nold, const float *xold, const float *yold, float *y2, int nnew, const float *xnew, float *ynew, float *p, float *q)
{
    const int noldm1 = nold - 1;
    int k, k1, k2, kold = 0;
    float ak = 0.f, bk = 0.f, ck = 0.f;
    float dxl = xold[2] - xold[1], dxr = xold[3] - xold[2];
    float dydxl = (yold[2] - yold[1]) / dxl, dydxr = (yold[3] - yold[2]) / dxr;
    const float rtdxc = 0.5f / (dxl + dxr);
    p[1] = rtdxc * (6.f * (dydxr - dydxl) - dxl * y2[1]);
    q[1] = -rtdxc * dxr;
    if (nold != 3) {
        k = 3;
        do {
            dxl = dxr; dydxl = dydxr;
            dxr = xold[k + 1] - xold[k];
            dydxr = (yold[k + 1] - yold[k]) / dxr;
            const float dxc = dxl + dxr;
            const float den = 1.f / (dxl * q[k - 2] + dxc + dxc);
            p[k - 1] = den * (6.f * (dydxr - dydxl) - dxl * p[k - 2]);
            q[k - 1] = -den * dxr;
            k = k + 1;
        } while (k < nold);
    }
    k = noldm1;
    do { y2[k] = p[k - 1] + q[k - 1] * y2[k + 1]; k = k - 1; } while (k > 1);
    for (k1 = 1; k1 <= nnew; ++k1) {
        const float xk = xnew[k1];
        int found = 0;
        for (k2 = 2; k2 <= nold; ++k2) if (xold[k2] > xk) { kold = k2 - 1; found = 1; break; }
        if (!found) { ynew[k1] = yold[nold]; continue; }
        if (k1 == 1 || k != kold) {
            k = kold;
            const float y2k = y2[k], y2kp1 = y2[k + 1], dx = xold[k + 1] - xold[k], rdx = 1.f / dx;
            ak = .1666667f * rdx * (y2kp1 - y2k);
            bk = 0.5f * y2k;
            ck = rdx * (yold[k + 1] - yold[k]) - .1666667f * dx * (y2kp1 + y2k + y2k);
        }
        const float x = xk - xold[k], xsq = x * x;
        ynew[k1] = ak * xsq * x + bk * xsq + ck * x + yold[k];
    }
}

/* one T(theta-e) table of BMJINIT (:1962-2014 coarse, :2020-2084 fine) */
static void bmj_ttbl_build(int kthm, int kpm, float thtop, float plow, float dp, float *the0, float *sthe, float *ttbl, float capa, float elocp)
{
    const float EPS = 1.E-9f;
    float told[BMJ_JTBQ + 1], theold[BMJ_JTBQ + 1], thenew[BMJ_JTBQ + 1], tnew[BMJ_JTBQ + 1], y2t[BMJ_JTBQ + 1], apt[BMJ_JTBQ + 1], aqt[BMJ_JTBQ + 1];
    const int kthm1 = kthm - 1;
    const float dth = (thtop - BMJ_THL) / (float)(kthm - 1);
    float p = plow - dp;
    for (int kp = 1; kp <= kpm; ++kp) {
        p = p + dp;
        float th = BMJ_THL - dth;
        for (int kth = 1; kth <= kthm; ++kth) {
            th = th + dth;
            const float ape = BMJ_HOST_POWF(1.E5f / p, capa);
            const float denom = th - BMJ_A4 * ape;
            float qs;
            if (denom > EPS) qs = BMJ_PQ0 / p * BMJ_HOST_EXPF(BMJ_A2 * (th - BMJ_A3 * ape) / denom);
            else qs = 0.f;
            told[kth] = th / ape;
            theold[kth] = th * BMJ_HOST_EXPF(elocp * qs / told[kth]);
        }
        const float the0k = theold[1], sthek = theold[kthm] - theold[1];
        theold[1] = 0.f; theold[kthm] = 1.f;
        for (int kth = 2; kth <= kthm1; ++kth) {
            theold[kth] = (theold[kth] - the0k) / sthek;
            if ((theold[kth] - theold[kth - 1]) < EPS) theold[kth] = theold[kth - 1] + EPS;
        }
        the0[kp - 1] = the0k; sthe[kp - 1] = sthek;
        thenew[1] = 0.f; thenew[kthm] = 1.f;
        const float dthe = 1.f / (float)(kthm - 1);
        for (int kth = 2; kth <= kthm1; ++kth) thenew[kth] = thenew[kth - 1] + dthe;
        y2t[1] = 0.f; y2t[kthm] = 0.f;
        bmj_spline(kthm, theold, told, y2t, kthm, thenew, tnew, apt, aqt);
        for (int kth = 1; kth <= kthm; ++kth) ttbl[(size_t)kthm * (kp - 1) + (kth - 1)] = tnew[kth];
    }
}

/* BMJINIT's tables (:1895-2084) into one block of BMJ_TABLE_FLOATS floats, in the order QS0, SQS, PTBL, THE0, STHE, TTBL, THE0Q,
 * STHEQ, TTBLQ (Fortran element order); cp, rd: what cu_driver.f90:236-237 passes */
static void bmj_build_tables(float *block, BmjTables *tb)
{
    const float EPS = 1.E-9f;
    const float cp = BMJ_CP, rd = BMJ_R, capa = rd / cp, elocp = BMJ_ELIWV / cp;
    float *QS0 = block, *SQS = QS0 + BMJ_JTB, *PTBL = SQS + BMJ_JTB, *THE0 = PTBL + BMJ_ITB * BMJ_JTB, *STHE = THE0 + BMJ_ITB;
    float *TTBL = STHE + BMJ_ITB, *THE0Q = TTBL + BMJ_JTB * BMJ_ITB, *STHEQ = THE0Q + BMJ_ITBQ, *TTBLQ = STHEQ + BMJ_ITBQ;
    float app[BMJ_JTB + 1], aqp[BMJ_JTB + 1], pnew[BMJ_JTB + 1], pold[BMJ_JTB + 1], qsnew[BMJ_JTB + 1], qsold[BMJ_JTB + 1], y2p[BMJ_JTB + 1];
    const int kthm = BMJ_JTB, kpm = BMJ_ITB, kpm1 = kpm - 1;
    const float dth = (BMJ_THH - BMJ_THL) / (float)(kthm - 1), dp = (BMJ_PH - BMJ_PL) / (float)(kpm - 1);
    float th = BMJ_THL - dth;
    for (int kth = 1; kth <= kthm; ++kth) {                                                            /* :1908-1958 */
        th = th + dth;
        float p = BMJ_PL - dp;
        for (int kp = 1; kp <= kpm; ++kp) {
            p = p + dp;
            const float ape = BMJ_HOST_POWF(100000.f / p, capa);
            const float denom = th - BMJ_A4 * ape;
            if (denom > EPS) qsold[kp] = BMJ_PQ0 / p * BMJ_HOST_EXPF(BMJ_A2 * (th - BMJ_A3 * ape) / denom);
            else qsold[kp] = 0.f;
            pold[kp] = p;
        }
        const float qs0k = qsold[1], sqsk = qsold[kpm] - qsold[1];
        qsold[1] = 0.f; qsold[kpm] = 1.f;
        for (int kp = 2; kp <= kpm1; ++kp) {
            qsold[kp] = (qsold[kp] - qs0k) / sqsk;
            if ((qsold[kp] - qsold[kp - 1]) < EPS) qsold[kp] = qsold[kp - 1] + EPS;
        }
        QS0[kth - 1] = qs0k; SQS[kth - 1] = sqsk;
        qsnew[1] = 0.f; qsnew[kpm] = 1.f;
        const float dqs = 1.f / (float)(kpm - 1);
        for (int kp = 2; kp <= kpm1; ++kp) qsnew[kp] = qsnew[kp - 1] + dqs;
        y2p[1] = 0.f; y2p[kpm] = 0.f;
        bmj_spline(kpm, qsold, pold, y2p, kpm, qsnew, pnew, app, aqp);
        for (int kp = 1; kp <= kpm; ++kp) PTBL[(size_t)BMJ_ITB * (kth - 1) + (kp - 1)] = pnew[kp];
    }
    bmj_ttbl_build(BMJ_JTB, BMJ_ITB, BMJ_THH, BMJ_PL, dp, THE0, STHE, TTBL, capa, elocp);
    bmj_ttbl_build(BMJ_JTBQ, BMJ_ITBQ, BMJ_THHQ, BMJ_PLQ, (BMJ_PH - BMJ_PLQ) / (float)(BMJ_ITBQ - 1), THE0Q, STHEQ, TTBLQ, capa, elocp);
    *tb = bmj_tables_at(block);
}
#endif

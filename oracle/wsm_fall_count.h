/* oracle/wsm_fall_count.h -- TEST INFRASTRUCTURE, NOT PRODUCT.
 * Branch counters of the semi-Lagrangian fall (nislfv_rain_plm / nislfv_rain_plm6) as oracle/wsm6_oracle.c and oracle/wsm3_oracle.c
 * restate it.  Off unless orc_wsm_fall_counters() was given an array of WFC_N 64-bit integers; integer bookkeeping only, so no
 * floating-point operation of the fall depends on it.  oracle/orc.py: WSM_FALL_COUNTERS holds the names in this order. */
#pragma once
enum {
    WFC_EMPTY,        /* columns skipped because allold <= 0 */
    WFC_COLUMNS,      /* columns that fell */
    WFC_LIM_TRIP,     /* levels where the deformation limiter trips (decfl > con1) */
    WFC_RE_EVAL,      /* levels evaluated with a wi(k+1) that the limiter had just changed */
    WFC_RE_TRIP,      /*   ... that then trip */
    WFC_RE_PASS,      /*   ... that then do not */
    WFC_SHAFT_TOP,    /* levels k >= 2 (1-based) with ww(k) == 0: wi(k) = ww(k-1) */
    WFC_EXIT_INTP,    /* levels left at 0 by `exit intp` */
    WFC_KT_EQ_KB,     /* kt == kb */
    WFC_KT_GT_0MID,   /* kt > kb, no whole arrival cell between them */
    WFC_KT_GT_MID,    /* kt > kb, one or more whole arrival cells between them */
    WFC_MAX_MID,      /* the largest count of such cells (a maximum, not a sum) */
    WFC_KT_LT_KB,     /* kt < kb: qn = 0 */
    WFC_REC_FLAT,     /* reconstruction flat because dip*dim <= 0 */
    WFC_REC_SLOPED,   /* reconstruction sloped */
    WFC_REC_CLIP,     /* reconstruction flattened because an edge value went negative */
    WFC_OUT_NONE,     /* rain-out: nothing */
    WFC_OUT_PARTIAL,  /* rain-out: the partial cell only */
    WFC_OUT_WHOLE,    /* rain-out: one or more whole cells */
    WFC_N
};
extern long long *g_wsm_fall_cnt;
#define WFC_ADD(i, n) do { if (g_wsm_fall_cnt) { _Pragma("omp atomic") g_wsm_fall_cnt[i] += (n); } } while (0)
#define WFC(i) WFC_ADD(i, 1)
#define WFC_MAX(i, n) do { if (g_wsm_fall_cnt) { _Pragma("omp critical(wfc_max)") { if (g_wsm_fall_cnt[i] < (n)) g_wsm_fall_cnt[i] = (n); } } } while (0)

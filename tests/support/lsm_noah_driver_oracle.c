/* TEST INFRASTRUCTURE: tests/support/lsm_noah_driver_oracle.c -- the CPU restatement of the Noah branch of lsm() around the call of
 * lsm_noah (lsm_driver.f90:1028-1030, :1144-1147, :1181-1187, :1207, :1280-1290, :1524-1527, surface_diagnostics) and of lsm_init's
 * statements for it (:566, :583-611, :992-997): the product's own cell header icar_amd/csrc/lsm_noah_driver_cell.h compiled for the
 * host (gcc -O2 -ffp-contract=off) with the C library's logf / expf / sqrtf.  Arrays are the reference's: (ims:ime, jms:jme) with
 * ims = jms = 1, the soil field (ims:ime, 1:4, jms:jme); the first-level fields are passed as (nx, ny) slices.  flags may be 0. */
#include <math.h>
#include <stddef.h>
#define LND_FN static inline
#define LND_LOGF logf
#define LND_EXPF expf
#define LND_SQRTF sqrtf
#include "../../icar_amd/csrc/lsm_noah_driver_cell.h"

/* lsm_init's part (icar_hip_lsm_noah_couple) over the memory rectangle */
void lnd_oracle_couple(int nx, int ny, const float *znt, const float *z1, const float *terrain, const float *t1, const float *qv1, const double *precip,
                       float *noah_z0, float *chs, float *chs2, float *curprecip, double *rainbl, float *t2, float *q2, float *z_atm, float *lnz,
                       float *base)
{
    for (size_t at = 0; at < (size_t)nx * ny; ++at) {
        noah_z0[at] = znt[at];
        chs[at] = 0.01f; chs2[at] = 0.01f; curprecip[at] = 0.0f;
        rainbl[at] = precip[at];
        t2[at] = t1[at]; q2[at] = qv1[at];
        z_atm[at] = z1[at] - terrain[at];
        lnd_exchange_terms(z_atm[at], znt[at], &lnz[at], &base[at]);
    }
}

/* ahead of water_simple and lsm_noah, over the memory rectangle.  flags: lnd_exchange's, 32 a land cell (QGH written), 64 sat_mr below
   273.15 K, 128 precipitation > 0 */
void lnd_oracle_pre(int nx, int ny, const float *u10, const float *v10, const float *tsk, const float *t1, const float *z_atm, const float *lnz,
                    const float *base, const float *t2, const float *psfc, const int *land_mask, const double *precip, const double *rainbl,
                    float *ri, float *chs, float *chs2, float *cqs2, float *qgh, float *curprecip, int *flags)
{
    for (size_t at = 0; at < (size_t)nx * ny; ++at) {
        int f;
        lnd_exchange(u10[at], v10[at], tsk[at], t1[at], z_atm[at], lnz[at], base[at], &ri[at], &chs[at], &f);
        chs2[at] = chs[at]; cqs2[at] = chs[at];
        if (land_mask[at] == LND_LC_LAND) {
            qgh[at] = lnd_sat_mr(t2[at], psfc[at]);
            f |= 32 | (t2[at] < 273.15f ? 64 : 0);
        }
        curprecip[at] = lnd_current_precipitation(precip[at], rainbl[at]);
        if (curprecip[at] > 0) f |= 128;
        if (flags) flags[at] = f;
    }
}

/* behind lsm_noah: the whole-array statements over the memory rectangle, surface_diagnostics on its..ite, jts..jte (1-based, inclusive).
   flags: lnd_surface_diagnostics', 8 inside the tile, 16 the max_swe clamp acted */
void lnd_oracle_post(int nx, int ny, int its, int ite, int jts, int jte, float max_swe, const float *z_atm, const float *znt, const float *emiss,
                     const float *tsk, const float *smois, const float *hfx, const float *qfx, const float *qsfc, const float *chs2, const float *cqs2,
                     const float *psfc, const double *precip, float *swe, float *lnz, float *base, float *lwup, float *smstot, float *t2, float *q2,
                     double *rainbl, int *flags)
{
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const size_t at = (size_t)j * nx + i, s = (size_t)j * 4 * nx + i;
            int f = swe[at] > max_swe ? 16 : 0, g = 0;
            swe[at] = lnd_max_swe(swe[at], max_swe);
            lnd_exchange_terms(z_atm[at], znt[at], &lnz[at], &base[at]);
            lwup[at] = lnd_longwave_up(emiss[at], tsk[at]);
            rainbl[at] = precip[at];
            smstot[at] = lnd_soil_totalmoisture(smois[s], smois[s + nx], smois[s + 2 * (size_t)nx], smois[s + 3 * (size_t)nx]);
            if (i + 1 >= its && i + 1 <= ite && j + 1 >= jts && j + 1 <= jte) {
                lnd_surface_diagnostics(hfx[at], qfx[at], tsk[at], qsfc[at], chs2[at], cqs2[at], psfc[at], &t2[at], &q2[at], &g);
                f |= g | 8;
            }
            if (flags) flags[at] = f;
        }
}

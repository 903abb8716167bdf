/* tests/support/ysu_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of the boundary-layer slot as it runs for boundarylayer =
 * kPBL_YSU: pbl_init's arrays (src/physics/pbl_driver.f90:127-194) and the YSU branch of pbl (:223-354) around da_sfc_wtq
 * (src/utilities/pbl_utilities.f90) and ysu / ysu2d / tridin (src/physics/pbl_ysu.f90).  The cell and column code is the product's own
 * header, icar_amd/csrc/ysu_column.h, compiled here for the host with gcc -O2 -ffp-contract=off against the host's libm;
 * tests/test_ysu_oracle.py holds it bit for bit to the compiled reference's vectors (tests/golden/ysu_*.npz, made by
 * tests/golden/make_golden_ysu.py).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j), the 2-D ones (ny, nx); its..kte are 1-based inclusive like the reference's;
 * the memory extents ims:ime, kms:kme, jms:jme are 1:nx, 1:nz, 1:ny and kts is 1. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#define YSU_EXPF expf
#define YSU_LOGF logf
#define YSU_POWF powf
#define YSU_ATANF atanf
#define YSU_SQRTF sqrtf
#define YSU_DIAG
#include "../../icar_amd/csrc/ysu_column.h"

#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))

int ysu_oracle_min_levels(void) { return YSU_MIN_LEVELS; }
int ysu_oracle_max_levels(void) { return YSU_MAX_LEVELS; }
int ysu_oracle_workspace_arrays(void) { return YSU_NARR; }

/* pbl_init, YSU branch (pbl_driver.f90:136-151): z_atm, gz1oz0, zol = 10, hol = 1000 over the memory */
void ysu_oracle_init(int nx, int nz, int ny, const float *z, const float *terrain, const float *z0, float *z_atm, float *gz1oz0, float *zol,
                     float *hol)
{
    for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const size_t c2 = (size_t)j * nx + i;
        z_atm[c2] = z[IX(i,0,j)] - terrain[c2];
        zol[c2] = 10.0f;
        hol[c2] = 1000.0f;
        gz1oz0[c2] = logf(z_atm[c2] / z0[c2]);
    }
}

/* pbl_driver.f90:227-254 over the memory: windspd with its floor, calc_Richardson_nr (atm_utilities.f90:1138), da_sfc_wtq */
void ysu_oracle_sfc(int nx, int nz, int ny, float dx, const float *u10, const float *v10, const float *t, const float *tskin, const float *z_atm,
                    const float *psfc, const float *tg, const float *p, const float *qc, const float *um, const float *vm, const float *z0,
                    const int *land_mask, const float *ustar, float *windspd, float *ri, float *psim, float *psih, float *regime)
{
    for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const size_t c2 = (size_t)j * nx + i, a = IX(i,0,j);
        float w = sqrtf(u10[c2] * u10[c2] + v10[c2] * v10[c2]);
        if (w == 0) w = 1e-5f;
        windspd[c2] = w;
        ri[c2] = 9.81f / t[a] * (t[a] - tskin[c2]) * z_atm[c2] / (w * w);
        ysu_sfc_cell(psfc[c2], tg[c2], p[a], t[a], qc[a], um[a], vm[a], z_atm[c2], z0[c2], (float)land_mask[c2], dx, ustar[c2],
                     regime + c2, psim + c2, psih + c2);
    }
}

/* call ysu(...) (pbl_driver.f90:257-323) on its..ite, jts..jte, levels 1..kte-1; the tendencies stay where ysu leaves them.
 * diag (may be NULL): (ny, nz, nx) ints, ysu_column's flags (level k at index k, the column's at index 0).  Returns 1 when the
 * level count is refused. */
int ysu_oracle_ysu(int nx, int nz, int ny, int its, int ite, int jts, int jte, int kte, float dt, const float *um, const float *vm, const float *t,
                   const float *qv, const float *qc, const float *qi, const float *p, const float *pint, const float *pi, const float *dz,
                   const float *psfc, const float *z0, const float *ustar, const int *land_mask, const float *hfx, const float *lh,
                   const float *tsk, const float *gz1oz0, const float *windspd, const float *ri, const float *psim, const float *psih,
                   const float *u10, const float *v10, float *tend_u, float *tend_v, float *tend_th, float *tend_qv, float *tend_qc,
                   float *tend_qi, float *exch_h, float *hol, float *hpbl, int *kpbl, int *diag)
{
    const int n = kte - 1;
    if (n < YSU_MIN_LEVELS || n > YSU_MAX_LEVELS || kte > nz) return 1;
    const int nl = n + 1;
    float *ws = (float *)malloc(sizeof(float) * YSU_NARR * (size_t)nl);
    int *dg = (int *)malloc(sizeof(int) * (size_t)(n + 1));
    if (!ws || !dg) return 1;
    for (int j = jts - 1; j < jte; j++) for (int i = its - 1; i < ite; i++) {
        const size_t a = IX(i,0,j), c2 = (size_t)j * nx + i;
        YsuCol c = { um + a, vm + a, t + a, qv + a, qc + a, qi + a, p + a, pint + a, pi + a, dz + a,
                     tend_u + a, tend_v + a, tend_th + a, tend_qv + a, tend_qc + a, tend_qi + a, exch_h + a };
        YsuSfc s = { psfc[c2], z0[c2], ustar[c2], (float)land_mask[c2], hfx[c2], lh[c2] / YSU_XLV, tsk[c2], gz1oz0[c2], windspd[c2], ri[c2],
                     psim[c2], psih[c2], u10[c2], v10[c2] };
        YsuOut o;
        ysu_column(c, (size_t)nx, n, dt, s, &o, ws, 1, nl, dg);
        hol[c2] = o.hol; hpbl[c2] = o.hpbl; kpbl[c2] = o.kpbl;
        if (diag) for (int k = 0; k <= n; k++) diag[IX(i,k,j)] = dg[k];
    }
    free(ws); free(dg);
    return 0;
}

/* pbl_driver.f90:343-354 over the memory: the four updates, then the six tendencies to zero */
void ysu_oracle_apply(int nx, int nz, int ny, float dt, float *qv, float *qc, float *th, float *qi, float *tend_u, float *tend_v, float *tend_th,
                      float *tend_qv, float *tend_qc, float *tend_qi)
{
    const size_t n3 = (size_t)nx * nz * ny;
    for (size_t a = 0; a < n3; a++) {
        qv[a] = qv[a] + tend_qv[a] * dt;
        qc[a] = qc[a] + tend_qc[a] * dt;
        th[a] = th[a] + tend_th[a] * dt;
        qi[a] = qi[a] + tend_qi[a] * dt;
        tend_qv[a] = 0; tend_th[a] = 0; tend_qc[a] = 0; tend_qi[a] = 0; tend_u[a] = 0; tend_v[a] = 0;
    }
}

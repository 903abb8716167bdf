/* tests/support/bmj_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of the convection slot as it runs for convection = kCU_BMJ:
 * convect (src/physics/cu_driver.f90:255-514) around BMJDRV / BMJ (src/physics/cu_bmj.f90), and BMJINIT's lookup tables.  The column
 * code is the product's own header, icar_amd/csrc/bmj_column.h, compiled here for the host with gcc -O2 -ffp-contract=off against
 * the host's libm (expf, powf); tests/test_bmj_oracle.py holds it bit for bit to the compiled reference's vectors
 * (tests/golden/cu_bmj_*.npz, made by tests/golden/make_golden_bmj.py).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j), the 2-D ones (ny, nx); its..kte are 1-based inclusive like the reference's;
 * the memory extents ims:ime, kms:kme, jms:jme are 1:nx, 1:nz, 1:ny.  kts is 1: BMJDRV's flip KFLIP = KTE+1-K maps K = KTS..KTE onto
 * KTS..KTE only then (with kts = 2 it reads DTDT(1) below the array's lower bound, cu_bmj.f90:248). */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#define BMJ_EXPF expf
#define BMJ_POWF powf
#define BMJ_WITH_TABLES
#include "../../icar_amd/csrc/bmj_column.h"

#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))
static float table_block[BMJ_TABLE_FLOATS];
static BmjTables tables;
static int have_tables = 0;
static void need_tables(void) { if (!have_tables) { bmj_build_tables(table_block, &tables); have_tables = 1; } }

int bmj_oracle_table_floats(void) { return BMJ_TABLE_FLOATS; }
int bmj_oracle_max_levels(void) { return BMJ_MAX_LEVELS; }
int bmj_oracle_workspace_arrays(void) { return BMJ_NARR; }
float bmj_oracle_avgefi(void) { return BMJ_AVGEFI; }
float bmj_oracle_efimn(void) { return BMJ_EFIMN; }
/* QS0, SQS, PTBL, THE0, STHE, TTBL, THE0Q, STHEQ, TTBLQ one behind the other, Fortran element order */
void bmj_oracle_tables(float *out) { need_tables(); for (int n = 0; n < BMJ_TABLE_FLOATS; n++) out[n] = table_block[n]; }

/* BMJDRV on its..ite, jts..jte, levels 1..kte-1 (cu_driver.f90:434-465).  kind (may be NULL): BMJ_NONE / BMJ_DEEP / BMJ_SHALLOW per column.
 * Returns 1 when the level count is refused. */
int bmj_oracle_drv(int nx, int nz, int ny, int its, int ite, int jts, int jte, int kte, float dt, const float *t, const float *qv,
                   const float *pmid, const float *pint, const float *pi, const float *rho, const float *dz, const int *land_mask,
                   float *cldefi, float *raincv, float *cutop, float *cubot, float *tend_th, float *tend_qv, int *kind)
{
    const int n = kte - 1;
    if (n < 2 || n > BMJ_MAX_LEVELS || kte > nz) return 1;
    need_tables();
    float *ws = (float *)malloc(sizeof(float) * BMJ_NARR * (size_t)n);
    if (!ws) return 1;
    for (int j = jts - 1; j < jte; j++) for (int i = its - 1; i < ite; i++) {
        const size_t a = IX(i,0,j), c2 = (size_t)j * nx + i;
        BmjCol c = { t + a, qv + a, pmid + a, pint + a, pi + a, rho + a, dz + a, tend_th + a, tend_qv + a };
        const int lm = land_mask[c2];
        const float xland = lm == 0 ? 2.0f : (float)lm;                  /* cu_driver.f90:139-140 */
        const int r = bmj_drv_column(c, (size_t)nx, n, dt, xland, cldefi + c2, raincv + c2, cutop + c2, cubot + c2, ws, 1, &tables);
        if (kind) kind[c2] = r;
    }
    free(ws);
    return 0;
}

/* x = x + tend*dt*fraction over all i and k of memory on one row (cu_driver.f90:489-492); tend == NULL: an array of zeros */
static void apply_row(int nx, int nz, int j, float *x, const float *tend, float dt, float fraction)
{
    for (int k = 0; k < nz; k++) for (int i = 0; i < nx; i++) {
        const size_t a = IX(i,k,j);
        x[a] = x[a] + (tend ? tend[a] : 0.0f) * dt * fraction;
    }
}

/* convect(domain, options, dt) for convection = kCU_BMJ, stochastic_cu = kNO_STOCHASTIC (cu_driver.f90:255-514) */
int bmj_oracle_convect(int nx, int nz, int ny, int its, int ite, int jts, int jte, int kte, float dt, const float *t, float *qv, float *th,
                       float *qc, float *qi, const float *pmid, const float *pint, const float *pi, const float *rho, const float *dz,
                       const int *land_mask, float *cldefi, float *raincv, float *cutop, float *cubot, float *tend_th, float *tend_qv,
                       double *acc_precip, float *acc_conv, float tendency_fraction, float f_qv, float f_qc, float f_th, float f_qi, int *kind)
{
    for (int j = jts - 1; j < jte; j++) {                                  /* :272-282 */
        for (int i = 0; i < nx; i++) raincv[(size_t)j * nx + i] = 0.0f;
        for (int k = 0; k < nz; k++) for (int i = 0; i < nx; i++) { tend_th[IX(i,k,j)] = 0.0f; tend_qv[IX(i,k,j)] = 0.0f; }
    }
    if (bmj_oracle_drv(nx, nz, ny, its, ite, jts, jte, kte, dt, t, qv, pmid, pint, pi, rho, dz, land_mask, cldefi, raincv, cutop, cubot,
                       tend_th, tend_qv, kind)) return 1;
    for (int j = jts - 1; j < jte; j++) {                                  /* :483-500 */
        if (tendency_fraction > 0) {
            if (f_qv > 0) apply_row(nx, nz, j, qv, tend_qv, dt, f_qv);
            if (f_qc > 0) apply_row(nx, nz, j, qc, NULL, dt, f_qc);
            if (f_th > 0) apply_row(nx, nz, j, th, tend_th, dt, f_th);
            if (f_qi > 0) apply_row(nx, nz, j, qi, NULL, dt, f_qi);
        }
        for (int i = 0; i < nx; i++) {
            const size_t c2 = (size_t)j * nx + i;
            acc_precip[c2] = acc_precip[c2] + raincv[c2];
            acc_conv[c2] = acc_conv[c2] + raincv[c2];
        }
    }
    return 0;
}

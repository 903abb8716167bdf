/* TEST INFRASTRUCTURE: tests/support/noah_oracle.c -- the CPU restatement of lsm_noah and LSM_NOAH_INIT as lsm_driver.f90 calls them:
 * the product's own cell header icar_amd/csrc/noah_column.h compiled for the host (gcc -O2 -ffp-contract=off), with the C library's
 * expf / exp2f / logf / log10f / powf and the branch counters of the coverage table switched on.  Arrays are the reference's: a field
 * of one value per cell is (ims:ime, jms:jme) with ims = jms = 1, a soil field (ims:ime, 1:4, jms:jme). */
#include <math.h>
#include <string.h>
#define NOAH_EXPF expf
#define NOAH_EXP2F exp2f
#define NOAH_LOGF logf
#define NOAH_LOG10F log10f
#define NOAH_POWF powf
#define NOAH_DIAG
#include "../../icar_amd/csrc/noah_column.h"

/* the order in which noah_oracle_run takes its arrays: every NOAH_ATM_FIELDS, NOAH_IN_FIELDS, NOAH_IO_FIELDS, NOAH_SOIL_FIELDS, then ivgtyp, isltyp */
const char *noah_oracle_fields(void)
{
#define NOAH_X(n) #n " "
    return NOAH_ATM_FIELDS(NOAH_X) NOAH_IN_FIELDS(NOAH_X) NOAH_IO_FIELDS(NOAH_X) NOAH_SOIL_FIELDS(NOAH_X) "ivgtyp isltyp";
#undef NOAH_X
}

int noah_oracle_sizeof_tables(void) { return (int)sizeof(NoahTables); }

/* lsm_noah on the tile its..ite, jts..jte (1-based, inclusive) of an nx x ny memory rectangle; diag may be 0 */
void noah_oracle_run(int nx, int ny, int its, int ite, int jts, int jte, float dt, int isurban, int isice, const NoahTables *T, void **f,
                     unsigned long long *diag)
{
    (void)ny;
    for (int j = jts - 1; j < jte; ++j)
        for (int i = its - 1; i < ite; ++i) {
            NoahCell c;
            unsigned long long d = 0;
            const size_t at = (size_t)j * nx + i;
            int n = 0;
#define NOAH_X(name) c.name = ((const float *)f[n++])[at];
            NOAH_ATM_FIELDS(NOAH_X)
            NOAH_IN_FIELDS(NOAH_X)
            NOAH_IO_FIELDS(NOAH_X)
#undef NOAH_X
#define NOAH_X(name) { const float *a = (const float *)f[n++]; for (int s = 0; s < NOAH_NSOIL; ++s) c.name[s] = a[((size_t)j * NOAH_NSOIL + s) * nx + i]; }
            NOAH_SOIL_FIELDS(NOAH_X)
#undef NOAH_X
            c.ivgtyp = ((const int *)f[n++])[at];
            c.isltyp = ((const int *)f[n++])[at];
            noah_cell(T, &c, dt, isurban, isice, &d);
            n = 0;
#define NOAH_X(name) n++;
            NOAH_ATM_FIELDS(NOAH_X)
            NOAH_IN_FIELDS(NOAH_X)
#undef NOAH_X
#define NOAH_X(name) ((float *)f[n++])[at] = c.name;
            NOAH_IO_FIELDS(NOAH_X)
#undef NOAH_X
#define NOAH_X(name) { float *a = (float *)f[n++]; for (int s = 0; s < NOAH_NSOIL; ++s) a[((size_t)j * NOAH_NSOIL + s) * nx + i] = c.name[s]; }
            NOAH_SOIL_FIELDS(NOAH_X)
#undef NOAH_X
            if (diag) diag[at] = d;
        }
}

/* LSM_NOAH_INIT's per-cell part on the tile; returns the number of cells with ISLTYP < 1 (the reference stops there) */
int noah_oracle_init(int nx, int ny, int its, int ite, int jts, int jte, int fndsnowh, const NoahTables *T, const int *ivgtyp, const int *isltyp,
                     const float *tslb, const float *smois, float *sh2o, float *snoalb, const float *snow, float *snowh, float *canwat,
                     unsigned long long *diag)
{
    int bad = 0;
    (void)ny;
    for (int j = jts - 1; j < jte; ++j)
        for (int i = its - 1; i < ite; ++i) {
            const size_t at = (size_t)j * nx + i;
            float st[NOAH_NSOIL], sm[NOAH_NSOIL], sw[NOAH_NSOIL];
            unsigned long long d = 0;
            for (int s = 0; s < NOAH_NSOIL; ++s) {
                const size_t a3 = ((size_t)j * NOAH_NSOIL + s) * nx + i;
                st[s] = tslb[a3]; sm[s] = smois[a3]; sw[s] = sh2o[a3];
            }
            bad += noah_init_cell(T, ivgtyp[at], isltyp[at], st, sm, sw, &snoalb[at], snow[at], &snowh[at], &canwat[at], fndsnowh, &d);
            for (int s = 0; s < NOAH_NSOIL; ++s) sh2o[((size_t)j * NOAH_NSOIL + s) * nx + i] = sw[s];
            if (diag) diag[at] = d;
        }
    return bad;
}

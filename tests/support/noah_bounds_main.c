/* tests/support/noah_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python): the
 * restatement of lsm_noah and LSM_NOAH_INIT (icar_amd/csrc/noah_column.h compiled for the host, through noah_oracle.c) under the address
 * and undefined-behaviour sanitizers.  The compiled reference checks no array bounds; this run is what says that the restatement -- and
 * with it the device code, which is the same header -- stays inside the extents the reference declares.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/noah_bounds_main.c -o noah_bounds -lm
 *   ./noah_bounds case.bin      the case tests/test_noah_bounds.py wrote (a fixture's inputs): lsm_init, then every carried call
 * Every table is its own allocation of exactly the reference's extent (NLUS = 50, NSLTYPE = 30, NSLOPE = 30 elements), every field of
 * exactly nx ny (soil: nx 4 ny) elements; the four-layer work arrays are locals of the header, each with its own red zone.  After the
 * case the program runs single cells whose categories sit at BOTH ENDS of every table (vegetation 1 and 50, soil 1 and 30; the rows a
 * table file leaves unfilled get a copy of a filled row first, so that the arithmetic stays finite).  Prints "checksum <sum of the
 * outputs' bit patterns>", which the test compares with the restatement run through python.  Exit status 0 = no finding. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "noah_oracle.c"

static void *g_all[4096];                                       /* every allocation, freed at the end */
static int g_nall;

static void *take(FILE *f, size_t n, size_t size)
{
    void *p = malloc(n * size);
    if (!p || g_nall == 4096 || fread(p, size, n, f) != n) { fprintf(stderr, "noah_bounds: short read\n"); exit(2); }
    g_all[g_nall++] = p;
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: noah_bounds case.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int h[7];                                                   /* nx, ny, calls, isurban, isice, fndsnowh, number of forcing arrays */
    float dt;
    if (fread(h, sizeof(int), 7, f) != 7 || fread(&dt, sizeof(float), 1, f) != 1) return 2;
    const int nx = h[0], ny = h[1], calls = h[2], isurban = h[3], isice = h[4], fnd = h[5], nforce = h[6];
    const size_t n2 = (size_t)nx * ny;
    NoahTables T;
    T.nrotbl = (const int *)take(f, NOAH_NLUS, sizeof(int));
    const float **veg[13] = {&T.snuptbl, &T.rstbl, &T.rgltbl, &T.hstbl, &T.maxalb, &T.emissmintbl, &T.emissmaxtbl, &T.laimintbl, &T.laimaxtbl,
                             &T.z0mintbl, &T.z0maxtbl, &T.albedomintbl, &T.albedomaxtbl};
    const float **soil[10] = {&T.bb, &T.drysmc, &T.f11, &T.maxsmc, &T.refsmc, &T.satpsi, &T.satdk, &T.satdw, &T.wltsmc, &T.qtz};
    for (int n = 0; n < 13; ++n) *veg[n] = (const float *)take(f, NOAH_NLUS, sizeof(float));
    for (int n = 0; n < 10; ++n) *soil[n] = (const float *)take(f, NOAH_NSLTYPE, sizeof(float));
    T.slope_data = (const float *)take(f, NOAH_NSLOPE, sizeof(float));
    float *gen = (float *)take(f, 13, sizeof(float));
    int *ints = (int *)take(f, 4, sizeof(int));
    T.topt_data = gen[0]; T.cmcmax_data = gen[1]; T.cfactr_data = gen[2]; T.rsmax_data = gen[3]; T.sbeta_data = gen[4]; T.fxexp_data = gen[5];
    T.csoil_data = gen[6]; T.salp_data = gen[7]; T.refdk_data = gen[8]; T.refkdt_data = gen[9]; T.frzk_data = gen[10]; T.zbot_data = gen[11];
    T.lvcoef_data = gen[12];
    T.bare = ints[0]; T.lucats = ints[1]; T.slcats = ints[2]; T.slpcats = ints[3];
    /* the fields in noah_oracle_fields()'s order: 5 + 12 + 32 of nx ny, 4 of nx 4 ny, 2 of nx ny integers */
    enum { N2 = 5 + 12 + 32, NS = 4, NF = N2 + NS + 2 };
    void *fld[NF];
    for (int n = 0; n < NF; ++n) fld[n] = take(f, n2 * (n >= N2 && n < N2 + NS ? NOAH_NSOIL : 1), 4);
    /* lsm_init: LSM_NOAH_INIT with canopy_water kept (lsm_driver.f90:672, :707); the positions are those of the field list */
    enum { P_SNOALB = 5 + 7, P_SNOW = 17 + 16, P_SNOWH = 17 + 17, P_CANWAT = 17 + 18, P_SMOIS = N2, P_TSLB = N2 + 1, P_SH2O = N2 + 2 };
    float *keep = (float *)malloc(n2 * sizeof(float));
    for (size_t n = 0; n < n2; ++n) keep[n] = ((float *)fld[P_CANWAT])[n];
    if (noah_oracle_init(nx, ny, 1, nx, 1, ny, fnd, &T, (const int *)fld[NF - 2], (const int *)fld[NF - 1], (const float *)fld[P_TSLB], (const float *)fld[P_SMOIS],
                         (float *)fld[P_SH2O], (float *)fld[P_SNOALB], (const float *)fld[P_SNOW], (float *)fld[P_SNOWH], (float *)fld[P_CANWAT], 0)) return 4;
    for (size_t n = 0; n < n2; ++n) ((float *)fld[P_CANWAT])[n] = keep[n];
    int *where = (int *)take(f, nforce, sizeof(int));           /* which fields a call's forcing replaces */
    for (int c = 0; c < calls; ++c) {
        for (int n = 0; n < nforce; ++n) fld[where[n]] = take(f, n2, 4);
        noah_oracle_run(nx, ny, 1, nx, 1, ny, dt, isurban, isice, &T, fld, 0);
    }
    uint64_t sum = 0;
    for (int n = 17; n < N2 + NS; ++n) {
        const uint32_t *p = (const uint32_t *)fld[n];
        for (size_t k = 0; k < n2 * (n >= N2 ? NOAH_NSOIL : 1); ++k) sum += p[k];
    }
    printf("checksum %llu\n", (unsigned long long)sum);
    /* both ends of every table: unfilled rows get row 10 (vegetation) / row 6 (soil) */
    for (int n = 0; n < 13; ++n) for (int v = T.lucats; v < NOAH_NLUS; ++v) ((float *)*veg[n])[v] = (*veg[n])[9];
    for (int v = T.lucats; v < NOAH_NLUS; ++v) ((int *)T.nrotbl)[v] = T.nrotbl[9];
    for (int n = 0; n < 10; ++n) for (int s = T.slcats; s < NOAH_NSLTYPE; ++s) ((float *)*soil[n])[s] = (*soil[n])[5];
    int ends = 0;
    for (int v = 1; v <= NOAH_NLUS; v += NOAH_NLUS - 1)
        for (int s = 1; s <= NOAH_NSLTYPE; s += NOAH_NSLTYPE - 1)
            for (size_t cell = 0; cell < n2; ++cell) {
                if (((float *)fld[4])[cell] > 1.5f) continue;   /* xland: a land cell */
                ((int *)fld[NF - 2])[cell] = v; ((int *)fld[NF - 1])[cell] = s;
                const int i = (int)(cell % nx) + 1, j = (int)(cell / nx) + 1;
                noah_oracle_init(nx, ny, i, i, j, j, fnd, &T, (const int *)fld[NF - 2], (const int *)fld[NF - 1], (const float *)fld[P_TSLB],
                                 (const float *)fld[P_SMOIS], (float *)fld[P_SH2O], (float *)fld[P_SNOALB], (const float *)fld[P_SNOW], (float *)fld[P_SNOWH],
                                 (float *)fld[P_CANWAT], 0);
                noah_oracle_run(nx, ny, i, i, j, j, dt, isurban, isice, &T, fld, 0);
                ++ends;
                break;
            }
    printf("table ends: %d cells, no finding\n", ends);
    free(keep);
    for (int n = 0; n < g_nall; ++n) free(g_all[n]);
    fclose(f);
    return 0;
}

/* tests/support/lsm_noah_driver_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python,
 * nothing runs on a GPU): the restatement of the Noah branch of lsm() around the call (icar_amd/csrc/lsm_noah_driver_cell.h through
 * lsm_noah_driver_oracle.c) under the address and undefined-behaviour sanitizers.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/lsm_noah_driver_bounds_main.c -o lnd_bounds -lm
 *   ./lnd_bounds
 * It runs lsm_init's statements, then two passes of the statements ahead of and behind lsm_noah, on a 3 x 3 and a 65 x 3 memory rectangle
 * with tiles that touch every edge (the whole rectangle, each single edge row / column, each corner cell, the one interior cell).  Every
 * array is its own allocation of exactly nx ny (the soil array nx 4 ny) elements, so that one element past any of them is a finding.
 * Prints "checksum <sum of the outputs' bit patterns>" per rectangle, which tests/test_lsm_noah_driver_bounds.py compares with the
 * restatement run through python on the same inputs.  Exit status 0 = no finding. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lsm_noah_driver_oracle.c"

static float *farr(size_t n, unsigned *seed, float lo, float hi)
{
    float *p = (float *)malloc(n * sizeof(float));
    if (!p) exit(2);
    for (size_t k = 0; k < n; ++k) { *seed = *seed * 1664525u + 1013904223u; p[k] = lo + (hi - lo) * (float)(*seed >> 8) / 16777216.0f; }
    return p;
}

static uint64_t bits(const float *p, size_t n) { uint64_t s = 0; for (size_t k = 0; k < n; ++k) { uint32_t u; memcpy(&u, p + k, 4); s += u; } return s; }

static uint64_t rectangle(int nx, int ny)
{
    const size_t n2 = (size_t)nx * ny;
    unsigned seed = 12345u + (unsigned)nx;
    float *znt = farr(n2, &seed, 0.01f, 0.5f), *terrain = farr(n2, &seed, 0.f, 800.f), *z1 = farr(n2, &seed, 820.f, 860.f), *t1 = farr(n2, &seed, 265.f, 285.f);
    float *qv1 = farr(n2, &seed, 1e-4f, 8e-3f), *u10 = farr(n2, &seed, -3.f, 3.f), *v10 = farr(n2, &seed, -3.f, 3.f), *tsk = farr(n2, &seed, 262.f, 288.f);
    float *psfc = farr(n2, &seed, 7e4f, 1e5f), *emiss = farr(n2, &seed, 0.9f, 1.f), *smois = farr(4 * n2, &seed, 0.1f, 0.45f), *hfx = farr(n2, &seed, -50.f, 300.f);
    float *qfx = farr(n2, &seed, -1e-5f, 1e-4f), *qsfc = farr(n2, &seed, 1e-4f, 8e-3f), *swe = farr(n2, &seed, 0.f, 80.f);
    float *z0 = farr(n2, &seed, 0, 0), *chs = farr(n2, &seed, 0, 0), *chs2 = farr(n2, &seed, 0, 0), *cqs2 = farr(n2, &seed, 0, 0), *cur = farr(n2, &seed, 0, 0);
    float *t2 = farr(n2, &seed, 0, 0), *q2 = farr(n2, &seed, 0, 0), *z_atm = farr(n2, &seed, 0, 0), *lnz = farr(n2, &seed, 0, 0), *base = farr(n2, &seed, 0, 0);
    float *ri = farr(n2, &seed, 0, 0), *qgh = farr(n2, &seed, 0, 0), *lwup = farr(n2, &seed, 0, 0), *smstot = farr(n2, &seed, 0, 0);
    double *precip = (double *)malloc(n2 * sizeof(double)), *rainbl = (double *)malloc(n2 * sizeof(double));
    int *mask = (int *)malloc(n2 * sizeof(int)), *fl = (int *)malloc(n2 * sizeof(int));
    if (!precip || !rainbl || !mask || !fl) exit(2);
    for (size_t k = 0; k < n2; ++k) { precip[k] = 100.0 + 0.37 * (double)k; mask[k] = 1 + (int)(k % 3 == 0); z1[k] = terrain[k] + 20.0f + (float)(k % 7); }
    u10[0] = v10[0] = 0.0f;                                              /* wind == 0 */
    lnd_oracle_couple(nx, ny, znt, z1, terrain, t1, qv1, precip, z0, chs, chs2, cur, rainbl, t2, q2, z_atm, lnz, base);
    const int tiles[][4] = {{1, nx, 1, ny}, {1, 1, 1, ny}, {nx, nx, 1, ny}, {1, nx, 1, 1}, {1, nx, ny, ny}, {1, 1, 1, 1}, {nx, nx, ny, ny}, {1, 1, ny, ny},
                            {nx, nx, 1, 1}, {2, nx - 1, 2, ny - 1}};
    for (int pass = 0; pass < 2; ++pass)
        for (size_t t = 0; t < sizeof tiles / sizeof tiles[0]; ++t) {
            for (size_t k = 0; k < n2; ++k) precip[k] += 0.25 * (double)((k + t) % 5);
            lnd_oracle_pre(nx, ny, u10, v10, tsk, t1, z_atm, lnz, base, t2, psfc, mask, precip, rainbl, ri, chs, chs2, cqs2, qgh, cur, fl);
            lnd_oracle_post(nx, ny, tiles[t][0], tiles[t][1], tiles[t][2], tiles[t][3], 40.0f, z_atm, znt, emiss, tsk, smois, hfx, qfx, qsfc, chs2, cqs2, psfc,
                            precip, swe, lnz, base, lwup, smstot, t2, q2, rainbl, pass ? fl : 0);
        }
    uint64_t sum = bits(ri, n2) + bits(chs, n2) + bits(qgh, n2) + bits(cur, n2) + bits(swe, n2) + bits(lnz, n2) + bits(base, n2) + bits(lwup, n2) +
                   bits(smstot, n2) + bits(t2, n2) + bits(q2, n2);
    float *all[] = {znt, terrain, z1, t1, qv1, u10, v10, tsk, psfc, emiss, smois, hfx, qfx, qsfc, swe, z0, chs, chs2, cqs2, cur, t2, q2, z_atm, lnz, base, ri, qgh,
                    lwup, smstot};
    for (size_t k = 0; k < sizeof all / sizeof all[0]; ++k) free(all[k]);
    free(precip); free(rainbl); free(mask); free(fl);
    return sum;
}

int main(void)
{
    printf("checksum 3x3 %llu\n", (unsigned long long)rectangle(3, 3));
    printf("checksum 65x3 %llu\n", (unsigned long long)rectangle(65, 3));
    printf("no finding\n");
    return 0;
}

/* tests/support/ysu_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python): the
 * restatement of the boundary-layer slot with kPBL_YSU (ysu_oracle.c, i.e. icar_amd/csrc/ysu_column.h compiled for the host) at EVERY
 * level count from 3 to 130 on a probe state, two carried calls each, under the address and undefined-behaviour sanitizers.  The
 * compiled reference checks no array bounds; this run is what says that the restatement -- and with it the device code, which is
 * the same header on a workspace of the same extents -- stays inside its arrays.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/ysu_bounds_main.c -o ysu_bounds -lm && ./ysu_bounds
 * Prints, per level count, the largest kpbl and the columns whose boundary layer is convective; exit status 0 = no finding.
 * profiles/r16_steps.md holds the result.  Every field is allocated with exactly nx nz ny values and the column workspace with exactly
 * YSU_NARR x (n + 1) floats (ysu_oracle_ysu), so an access outside level 1..n+1 of any array lands in a red zone or in a neighbouring
 * array's first / last level and is caught either by the sanitizer or by the bit-for-bit comparison with the reference's vectors
 * (tests/test_ysu_oracle.py).  Level counts below 3 and above 129 must be refused. */
#include <stdio.h>
#include <string.h>
#include "ysu_oracle.c"

enum { NX = 24, NY = 6 };

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (*s >> 8) / 16777216.0; }
static float *fnew(size_t n) { return (float *)calloc(n, sizeof(float)); }

int main(void)
{
    int bad = 0;
    for (int nz = 1; nz <= 131; nz++) {
        const int nx = NX, ny = NY;
        const size_t n3 = (size_t)nx * nz * ny, n2 = (size_t)nx * ny;
        float *um = fnew(n3), *vm = fnew(n3), *t = fnew(n3), *th = fnew(n3), *qv = fnew(n3), *qc = fnew(n3), *qi = fnew(n3), *p = fnew(n3),
              *pint = fnew(n3), *pi = fnew(n3), *dz = fnew(n3), *z = fnew(n3), *exch = fnew(n3), *tu = fnew(n3), *tv = fnew(n3), *tth = fnew(n3),
              *tqv = fnew(n3), *tqc = fnew(n3), *tqi = fnew(n3);
        float *terrain = fnew(n2), *z0 = fnew(n2), *psfc = fnew(n2), *tsk = fnew(n2), *tg = fnew(n2), *hfx = fnew(n2), *lh = fnew(n2), *u10 = fnew(n2),
              *v10 = fnew(n2), *ust = fnew(n2), *z_atm = fnew(n2), *gz = fnew(n2), *zol = fnew(n2), *hol = fnew(n2), *wspd = fnew(n2), *ri = fnew(n2),
              *psim = fnew(n2), *psih = fnew(n2), *regime = fnew(n2), *hpbl = fnew(n2);
        int *lm = (int *)calloc(n2, sizeof(int)), *kpbl = (int *)calloc(n2, sizeof(int));
        unsigned seed = 4321u + nz;
        double wsum = 0;
        for (int k = 0; k < nz; k++) wsum += 0.4 + 1.6 * k / nz;
        const double lid = nz < 20 ? 4000.0 : 12000.0;
        for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
            const size_t c2 = (size_t)j * nx + i;
            const int stable = j >= ny / 2;
            const double th0 = 285.0 + 15.0 * i / (nx - 1), zml = 200.0 + 2300.0 * frand(&seed);
            double pk = 96000.0 + 3000.0 * frand(&seed), zlo = 0;
            terrain[c2] = (float)(300.0 * frand(&seed));
            lm[c2] = frand(&seed) < 0.3 ? 2 : 1;
            z0[c2] = (float)(lm[c2] == 2 ? 2e-4 + 8e-4 * frand(&seed) : 0.03 + 0.5 * frand(&seed));
            psfc[c2] = (float)pk;
            const double spd = frand(&seed) < 0.1 ? 0.0 : 0.5 + 12.0 * frand(&seed), dir = 6.28 * frand(&seed);
            for (int k = 0; k < nz; k++) {
                const size_t a = IX(i,k,j);
                const double d = lid * (0.4 + 1.6 * k / nz) / wsum * (0.985 + 0.015 * frand(&seed)), zm = zlo + 0.5 * d;
                double theta = stable ? th0 + 0.02 * (zm < 400.0 ? zm : 400.0) + 0.004 * (zm > 400.0 ? zm - 400.0 : 0.0)
                                      : th0 + (zm > zml ? 1.5 + 0.005 * (zm - zml) : 0.0);
                theta += 0.6 * (frand(&seed) < 0.12) + 0.04 * (frand(&seed) - 0.5);
                double T = theta * pow(pk / 1e5, 287.058 / 1012.0);
                const double ptop = pk * exp(-9.81 * d / (287.058 * T)), pm = sqrt(pk * ptop);
                T = theta * pow(pm / 1e5, 287.058 / 1012.0);
                const double es = 610.78 * exp(17.2693882 * (T - 273.16) / (T - 35.86));
                double q = 0.6 * (zm < zml ? 1.0 : exp(-(zm - zml) / 2500.0)) * 0.622 * es / (pm - es > 1.0 ? pm - es : 1.0); if (q < 1e-7) q = 1e-7;
                const double prof = log(zm / z0[c2] + 1.0) / log(1000.0 / z0[c2] + 1.0);
                dz[a] = (float)d; z[a] = (float)(zm + terrain[c2]); p[a] = (float)pm; pint[a] = (float)pk; t[a] = (float)T; qv[a] = (float)q;
                pi[a] = (float)pow(p[a] / 1e5, 287.058 / 1012.0); th[a] = t[a] / pi[a];
                um[a] = (float)(spd * prof * cos(dir) + 2.0 * (frand(&seed) - 0.5)); vm[a] = (float)(spd * prof * sin(dir) + (frand(&seed) - 0.5));
                qc[a] = (zm > 800.0 && zm < 2400.0 && (i % 3) == 0) ? (float)(3e-4 * frand(&seed)) : 0.0f;
                qi[a] = (T < 265.0 && (i % 3) == 0) ? (float)(1e-4 * frand(&seed)) : 0.0f;
                pk = ptop; zlo += d;
            }
            const size_t a1 = IX(i,0,j);
            const double z1 = 0.5 * dz[a1], lw = log(10.0 / z0[c2]) / log(z1 / z0[c2] + 1.0);
            u10[c2] = spd == 0.0 ? 0.0f : (float)(um[a1] * lw); v10[c2] = spd == 0.0 ? 0.0f : (float)(vm[a1] * lw);
            ust[c2] = (float)(0.03 + 0.41 * hypot(um[a1], vm[a1]) / log(z1 / z0[c2] + 1.0));
            tsk[c2] = t[a1] + (float)(stable ? -(0.5 + 6.0 * frand(&seed)) : 0.5 + 8.0 * frand(&seed));
            tg[c2] = tsk[c2] + (float)(0.6 * (frand(&seed) - 0.5));
            hfx[c2] = (float)(stable ? -(3.0 + 50.0 * frand(&seed)) : 20.0 + 700.0 * frand(&seed));
            lh[c2] = (float)(stable ? 10.0 * frand(&seed) : 20.0 + 400.0 * frand(&seed));
        }
        ysu_oracle_init(nx, nz, ny, z, terrain, z0, z_atm, gz, zol, hol);
        const int must_refuse = nz < YSU_MIN_LEVELS + 1 || nz > YSU_MAX_LEVELS + 1;
        int kmax = 0, conv = 0, refused = 0;
        for (int call = 0; call < 2 && !refused; call++) {
            const float dt = 30.0f + 45.0f * call;
            if (call) for (size_t a = 0; a < n3; a++) t[a] = th[a] * pi[a];
            ysu_oracle_sfc(nx, nz, ny, 2000.0f, u10, v10, t, tsk, z_atm, psfc, tg, p, qc, um, vm, z0, lm, ust, wspd, ri, psim, psih, regime);
            refused = ysu_oracle_ysu(nx, nz, ny, 2, nx - 1, 2, ny - 1, nz, dt, um, vm, t, qv, qc, qi, p, pint, pi, dz, psfc, z0, ust, lm, hfx, lh, tsk, gz,
                                     wspd, ri, psim, psih, u10, v10, tu, tv, tth, tqv, tqc, tqi, exch, hol, hpbl, kpbl, NULL);
            if (refused) break;
            for (size_t a = 0; a < n3; a++)
                if (!(tth[a] == tth[a]) || !(tqv[a] == tqv[a]) || !(tu[a] == tu[a]) || !(exch[a] == exch[a])) { printf("%d levels: NaN\n", nz); bad = 1; break; }
            if (call == 0) for (size_t c2 = 0; c2 < n2; c2++) { if (kpbl[c2] > kmax) kmax = kpbl[c2]; conv += kpbl[c2] > 1 && ri[c2] <= 0; }
            ysu_oracle_apply(nx, nz, ny, dt, qv, qc, th, qi, tu, tv, tth, tqv, tqc, tqi);
        }
        if (refused != must_refuse) { printf("%3d levels: refused = %d, expected %d\n", nz, refused, must_refuse); bad = 1; }
        else if (refused) printf("%3d levels: refused, as it must be\n", nz);
        else printf("%3d levels: largest kpbl %3d, convective columns %3d of %d\n", nz, kmax, conv, (nx - 2) * (ny - 2));
        float *all3[] = {um, vm, t, th, qv, qc, qi, p, pint, pi, dz, z, exch, tu, tv, tth, tqv, tqc, tqi};
        float *all2[] = {terrain, z0, psfc, tsk, tg, hfx, lh, u10, v10, ust, z_atm, gz, zol, hol, wspd, ri, psim, psih, regime, hpbl};
        for (size_t m = 0; m < sizeof all3 / sizeof *all3; m++) free(all3[m]);
        for (size_t m = 0; m < sizeof all2 / sizeof *all2; m++) free(all2[m]);
        free(lm); free(kpbl);
    }
    printf(bad ? "FINDINGS\n" : "levels 3..129: no sanitizer finding, no NaN; 1, 2, 130, 131 levels refused\n");
    return bad;
}

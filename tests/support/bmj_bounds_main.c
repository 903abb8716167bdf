/* tests/support/bmj_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python): the
 * restatement of the convection slot (bmj_oracle.c, i.e. icar_amd/csrc/bmj_column.h compiled for the host) at EVERY level count
 * from 3 to 90 on the probe sounding, three carried calls each, under the address and undefined-behaviour sanitizers.  The
 * compiled reference checks no array bounds; this run is what says that the restatement -- and with it the device code, which is
 * the same header on a workspace of the same extents -- stays inside its arrays.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/bmj_bounds_main.c -o bmj_bounds -lm && ./bmj_bounds
 * Prints, per level count, the deep / shallow / quiet columns of the first call; exit status 0 = no finding.  profiles/r14_steps.md
 * holds the result.  The column workspace is allocated with exactly BMJ_NARR x n floats (bmj_oracle_drv), so any access outside
 * level 1..n of any array lands in a red zone or in a neighbouring array's first / last level and is caught either by the
 * sanitizer or by the bit-for-bit comparison with the reference's vectors (tests/test_bmj_oracle.py). */
#include <stdio.h>
#include <string.h>
#include "bmj_oracle.c"

enum { NX = 32, NY = 24 };

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (*s >> 8) / 16777216.0; }

int main(void)
{
    int bad = 0;
    for (int nz = 3; nz <= 90; nz++) {
        const int nx = NX, ny = NY;
        const size_t n3 = (size_t)nx * nz * ny, n2 = (size_t)nx * ny;
        float *f = calloc(12 * n3 + 6 * n2, sizeof(float));
        float *t = f, *qv = t + n3, *th = qv + n3, *qc = th + n3, *qi = qc + n3, *pmid = qi + n3, *pint = pmid + n3, *pi = pint + n3,
              *rho = pi + n3, *dz = rho + n3, *tth = dz + n3, *tqv = tth + n3, *cld = tqv + n3, *rain = cld + n2, *top = rain + n2,
              *bot = top + n2, *accc = bot + n2;
        double *acc = calloc(n2, sizeof(double));
        int *lm = calloc(n2, sizeof(int)), *kind = calloc(n2, sizeof(int));
        unsigned seed = 12345u + nz;
        double wsum = 0;
        for (int k = 0; k < nz; k++) wsum += 0.5 + (double)k / nz;
        for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
            const double fi = (double)i / (nx - 1), fj = (double)j / (ny - 1);
            const double tsfc = 284.0 + 22.0 * fi, rh0 = 0.25 + 0.72 * fj, H = 3000.0 + 4000.0 * fi;
            const double cap = ((i + 2 * j) % 3 == 0) ? 3.0 + 6.0 * frand(&seed) : 0.0, zinv = 2200.0 + 1200.0 * frand(&seed);
            double p = 97800.0 + 2200.0 * frand(&seed), zlo = 0;
            lm[(size_t)j * nx + i] = (frand(&seed) < 0.05) ? 0 : 1 + (i + j) % 2;
            cld[(size_t)j * nx + i] = 0.6f;
            for (int k = 0; k < nz; k++) {
                const size_t a = IX(i,k,j);
                const double d = 16000.0 * (0.5 + (double)k / nz) / wsum * (0.985 + 0.015 * frand(&seed)), z = zlo + 0.5 * d;
                double T = tsfc - 0.0065 * z; if (T < 210.0) T = 210.0;
                T += cap * exp(-((z - zinv) / 900.0) * ((z - zinv) / 900.0)) + 0.1 * (frand(&seed) - 0.5);
                const double ptop = p * exp(-9.81 * d / (287.058 * T)), pm = sqrt(p * ptop);
                const double rh = rh0 * (z < 1500.0 ? 1.0 : exp(-(z - 1500.0) / H));
                const double es = 610.78 * exp(17.2693882 * (T - 273.16) / (T - 35.86));
                double q = rh * 0.622 * es / (pm - es > 1.0 ? pm - es : 1.0); if (q < 1e-7) q = 1e-7;
                dz[a] = (float)d; t[a] = (float)T; pmid[a] = (float)pm; pint[a] = (float)p; qv[a] = (float)q;
                pi[a] = (float)pow(pmid[a] / 1e5, 287.058 / 1012.0); th[a] = t[a] / pi[a]; rho[a] = pmid[a] / (287.058f * t[a]);
                p = ptop; zlo += d;
            }
        }
        int deep = 0, shallow = 0, none = 0;
        for (int call = 0; call < 3; call++) {
            if (call) for (size_t a = 0; a < n3; a++) t[a] = th[a] * pi[a];
            if (bmj_oracle_convect(nx, nz, ny, 2, nx - 1, 2, ny - 1, nz, 20.0f * (call + 1), t, qv, th, qc, qi, pmid, pint, pi, rho, dz, lm, cld, rain,
                                   top, bot, tth, tqv, acc, accc, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, kind)) { printf("%d levels: refused\n", nz); bad = 1; break; }
            if (call == 0) for (size_t c2 = 0; c2 < n2; c2++) { deep += kind[c2] == BMJ_DEEP; shallow += kind[c2] == BMJ_SHALLOW; }
            for (size_t a = 0; a < n3; a++) if (!(tth[a] == tth[a]) || !(tqv[a] == tqv[a]) || !(th[a] == th[a])) { printf("%d levels: NaN\n", nz); bad = 1; break; }
        }
        none = (nx - 2) * (ny - 2) - deep - shallow;
        printf("%2d levels: deep %3d shallow %3d quiet %3d\n", nz, deep, shallow, none);
        free(f); free(acc); free(lm); free(kind);
    }
    printf(bad ? "FINDINGS\n" : "levels 3..90: no sanitizer finding, no NaN\n");
    return bad;
}

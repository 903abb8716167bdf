/* tests/support/tiedtke_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python): the
 * restatement of CU_TIEDTKE (tiedtke_oracle.c, i.e. icar_amd/csrc/tiedtke_column.h compiled for the host) on a probe state under the
 * address and undefined-behaviour sanitizers.  The compiled reference checks no array bounds; this run is what says that the
 * restatement -- and with it the device code, which is the same header on a workspace of the same extents -- stays inside its arrays.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/tiedtke_bounds_main.c -o tdk_bounds -lm
 *   ./tdk_bounds        every model level count from TDK_MIN_LEVELS + 1 to 130, two carried calls each; 130 must be refused
 *   ./tdk_bounds N      N model levels alone WITHOUT the refusal (tdk_column called directly): how tests/test_tiedtke_bounds.py
 *                       finds the smallest count without a finding, which is the refusal threshold of the library
 * Every field is allocated with exactly nx nz ny values and the column workspace with exactly TDK_NARR x (n + 2) floats, so an access
 * outside a column's levels lands in a red zone or in a neighbouring array and is caught by the sanitizer or by the bit-for-bit
 * comparison with the reference's vectors (tests/test_tiedtke_oracle.py).  Exit status 0 = no finding, no NaN. */
#include <stdio.h>
#include <string.h>
#include "tiedtke_oracle.c"

enum { NX = 24, NY = 6 };

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (*s >> 8) / 16777216.0; }
static float *fnew(size_t n) { return (float *)calloc(n, sizeof(float)); }

static int run(int nz, int direct)
{
    const int nx = NX, ny = NY;
    const size_t n3 = (size_t)nx * nz * ny, n2 = (size_t)nx * ny;
    float *t = fnew(n3), *qv = fnew(n3), *qc = fnew(n3), *qi = fnew(n3), *pi = fnew(n3), *rho = fnew(n3), *w = fnew(n3), *dz = fnew(n3),
          *p = fnew(n3), *pint = fnew(n3), *tth = fnew(n3), *tqv = fnew(n3), *tqc = fnew(n3), *tqi = fnew(n3);
    float *xland = fnew(n2), *rain = fnew(n2), *prate = fnew(n2), *znu = fnew((size_t)nz);
    int *ktype = (int *)calloc(n2, sizeof(int));
    unsigned seed = 8765u + nz;
    double wsum = 0;
    int bad = 0, conv = 0, wet = 0;
    for (int k = 0; k < nz; k++) { wsum += 0.5 + (double)k / nz; znu[k] = (float)((nz - k - 0.5) / nz); }
    for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const size_t c2 = (size_t)j * nx + i;
        const double tsfc = 284.0 + 22.0 * i / (nx - 1), base = 1500.0 + 2500.0 * frand(&seed), depth = 1500.0 + 6000.0 * frand(&seed);
        const double rhm = 0.78 + 0.22 * frand(&seed), wamp = -0.05 + 2.5 * frand(&seed);
        const int moist = frand(&seed) < 0.6;
        double pk = 97800.0 + 2200.0 * frand(&seed) - (j % 2 ? 25000.0 * i / (nx - 1) : 0.0), zlo = 0;
        xland[c2] = (i + j) % 2 ? 2.0f : 1.0f;
        for (int k = 0; k < nz; k++) {
            const size_t a = IX(i,k,j);
            const double d = 16000.0 * (0.5 + (double)k / nz) / wsum * (0.985 + 0.015 * frand(&seed)), zm = zlo + 0.5 * d;
            double T = tsfc - 0.0065 * zm; if (T < 210.0) T = 210.0;
            const double ptop = pk * exp(-9.81 * d / (287.058 * T)), pm = sqrt(pk * ptop);
            const double es = 610.78 * exp(17.269 * (T - 273.16) / (T - 35.86));
            const double qs = 0.622 * es / (pm - 0.378 * es > 1.0 ? pm - 0.378 * es : 1.0);
            double rh = 0.35 * (zm < 1500.0 ? 1.0 : exp(-(zm - 1500.0) / 4000.0));
            if (moist && zm > base && zm < base + depth) rh = rhm;
            double q = rh * qs / (1.0 - rh * qs); if (q < 1e-7) q = 1e-7;
            double s = zlo / 12000.0; if (s > 1.0) s = 1.0;
            dz[a] = (float)d; p[a] = (float)pm; pint[a] = (float)pk; t[a] = (float)T; qv[a] = (float)q;
            pi[a] = (float)pow(pm / 1e5, 287.058 / 1012.0); rho[a] = (float)(pm / (287.058 * T));
            w[a] = (float)((moist ? wamp : -0.02) * sin(3.14159265 * s));
            qc[a] = frand(&seed) < 0.2 ? (float)(3e-4 * frand(&seed)) : 0.0f;
            qi[a] = frand(&seed) < 0.1 ? (float)(1e-4 * frand(&seed)) : 0.0f;
            pk = ptop; zlo += d;
        }
    }
    for (int call = 0; call < 2; call++) {
        const float dt = call ? 120.0f : 60.0f;
        if (direct) {
            const int n = nz - 1;
            const size_t nl = (size_t)n + 2;
            float *ws = fnew(TDK_NARR * nl);
            for (int j = 0; j < ny; j++) {
                const int lt = tdk_leveltop(pint + IX(0,0,j), (size_t)nx, n);
                for (int i = 0; i < nx; i++) {
                    const size_t a = IX(i,0,j), c2 = (size_t)j * nx + i;
                    TdkIn in = { t + a, qv + a, qc + a, qi + a, pi + a, rho + a, w + a, dz + a, p + a, pint + a, (size_t)nx };
                    int dg = 0;
                    rain[c2] = tdk_column(in, n, (int)fabsf(xland[c2] - 2.f), lt, znu, 1, dt, ws, 1, nl, tth + a, tqv + a, tqc + a, tqi + a, (size_t)nx,
                                          ktype + c2, &dg);
                }
            }
            free(ws);
        } else {
            const int rc = tiedtke_oracle_run(nx, nz, ny, 1, nx, 1, ny, nz, dt, t, qv, qc, qi, pi, rho, w, dz, p, pint, xland, znu, tth, tqv, tqc, tqi,
                                              rain, prate, ktype, NULL, 0);
            if (rc) {
                if (nz - 1 > TDK_MAX_LEVELS) { printf("%d levels: refused, as it must be\n", nz); break; }
                printf("%d levels: REFUSED\n", nz); bad = 1; break;
            }
            if (nz - 1 > TDK_MAX_LEVELS) { printf("%d levels: NOT refused\n", nz); bad = 1; }
        }
        for (size_t a = 0; a < n3; a++) {
            if (!(tth[a] == tth[a]) || !(tqv[a] == tqv[a]) || !(tqc[a] == tqc[a]) || !(tqi[a] == tqi[a])) bad = 1;
            const float d = dt;                                                   /* carry: every fraction 1 */
            qv[a] = qv[a] + tqv[a] * d; qc[a] = qc[a] + tqc[a] * d; qi[a] = qi[a] + tqi[a] * d; t[a] = t[a] + tth[a] * pi[a] * d;
        }
        for (size_t c = 0; c < n2; c++) { if (!(rain[c] == rain[c])) bad = 1; conv += ktype[c] == 3; wet += rain[c] > 0; }
        if (call == 1) printf("%d levels: %d convective columns, %d with precipitation over two calls%s\n", nz, conv, wet, bad ? "  NaN!" : "");
    }
    free(t); free(qv); free(qc); free(qi); free(pi); free(rho); free(w); free(dz); free(p); free(pint); free(tth); free(tqv); free(tqc); free(tqi);
    free(xland); free(rain); free(prate); free(znu); free(ktype);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        const int nz = atoi(argv[1]);
        const int bad = run(nz, 1);
        printf("%d levels without the refusal: %s\n", nz, bad ? "NaN" : "no sanitizer finding, no NaN");
        return bad;
    }
    int bad = 0;
    for (int nz = TDK_MIN_LEVELS + 1; nz <= 130; nz++) bad |= run(nz, 0);
    if (!bad) printf("levels %d..129: no sanitizer finding, no NaN; 130 levels refused\n", TDK_MIN_LEVELS + 1);
    return bad;
}

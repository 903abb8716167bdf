/* tests/support/nsas_bounds_main.c -- TEST INFRASTRUCTURE, a stand-alone program (not a pytest; nothing is loaded into python): the
 * restatement of cu_nsas (icar_amd/csrc/nsas_column.h compiled for the host) on a probe state under the address and undefined-behaviour
 * sanitizers.  The compiled reference checks no array bounds; this run is what says that the restatement -- and with it the device
 * code, which is the same header -- stays inside the extents the reference declares.
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/support/nsas_bounds_main.c -o nsas_bounds -lm
 *   ./nsas_bounds        every scheme level count from NSAS_MIN_LEVELS to 129 model levels, two carried calls each
 *   ./nsas_bounds N      N scheme levels alone (no refusal is in the way here): how tests/test_nsas_bounds.py finds the smallest count
 *                        without a finding, which is the refusal threshold of the library
 * NSAS_WS is replaced by an accessor: every level array of a column is its own allocation of exactly the reference's extent
 * (kts:kte, zi kts:kte+1), and an index outside it ends the program with the array and the index.  The model's fields are allocated
 * with exactly nx nz ny values.  The workspace arrays are filled with NSAS_BOUNDS_FILL before each column; the test runs the program
 * built with two patterns and compares the printed checksums.  Exit status 0 = no finding, no NaN. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stddef.h>

#ifndef NSAS_BOUNDS_FILL
#define NSAS_BOUNDS_FILL 0x7FC00000u
#endif
static float *g_arr[64];
static int g_n;
static float *nsas_at(int a, long k);
#define NSAS_WS(a, k) (*nsas_at((a), (long)(k)))
#define NSAS_EXPF expf
#define NSAS_POWF powf
#define NSAS_SQRTF sqrtf
#include "../../icar_amd/csrc/nsas_column.h"

static float *nsas_at(int a, long k)
{
    const int hi = a == NSAS_ZI ? g_n + 1 : g_n;
    if (k < 1 || k > hi) {
        fprintf(stderr, "FINDING: workspace array %d read or written at level %ld outside 1..%d (%d scheme levels)\n", a, k, hi, g_n);
        exit(3);
    }
    return &g_arr[a][k - 1];
}

#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))
enum { NX = 24, NY = 6 };

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (*s >> 8) / 16777216.0; }
static float *fnew(size_t n) { return (float *)calloc(n, sizeof(float)); }

static int run(int nz, double *sum)
{
    const int nx = NX, ny = NY, n = nz - 1;
    const size_t n3 = (size_t)nx * nz * ny, n2 = (size_t)nx * ny;
    float *t = fnew(n3), *qv = fnew(n3), *qc = fnew(n3), *qi = fnew(n3), *pi = fnew(n3), *rho = fnew(n3), *w = fnew(n3), *dz = fnew(n3),
          *p = fnew(n3), *pint = fnew(n3), *u = fnew(n3), *v = fnew(n3), *tth = fnew(n3), *tqv = fnew(n3), *tqc = fnew(n3), *tqi = fnew(n3);
    float *xland = fnew(n2), *hfx = fnew(n2), *qfx = fnew(n2), *hpbl = fnew(n2), *rain = fnew(n2), *prate = fnew(n2), *hbot = fnew(n2), *htop = fnew(n2);
    unsigned seed = 4321u + nz;
    const unsigned fill = NSAS_BOUNDS_FILL;
    double wsum = 0;
    int bad = 0, deep = 0, shallow = 0;
    g_n = n;
    for (int a = 0; a < NSAS_NARR; a++) g_arr[a] = (float *)malloc(sizeof(float) * (size_t)(a == NSAS_ZI ? n + 1 : n));
    for (int k = 0; k < nz; k++) wsum += 0.5 + (double)k / nz;
    for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        const size_t c2 = (size_t)j * nx + i;
        const double tsfc = 284.0 + 22.0 * i / (nx - 1), wamp = -0.05 + 2.5 * frand(&seed), rh0 = 0.3 + 0.67 * j / (ny - 1);
        const double H = 3000.0 + 4000.0 * frand(&seed), sh = 4e-3 * frand(&seed);
        double pk = 97800.0 + 2200.0 * frand(&seed) - (j % 2 ? 25000.0 * i / (nx - 1) : 0.0), zlo = 0;
        xland[c2] = (i + j) % 2 ? 2.0f : 1.0f;
        hfx[c2] = (float)(frand(&seed) < 0.2 ? -40.0 * frand(&seed) : 350.0 * frand(&seed));
        qfx[c2] = (float)(400.0 * frand(&seed)) / 2260000.0f;
        hpbl[c2] = (float)(300.0 + 2200.0 * frand(&seed));
        for (int k = 0; k < nz; k++) {
            const size_t a = IX(i,k,j);
            const double d = 16000.0 * (0.5 + (double)k / nz) / wsum * (0.985 + 0.015 * frand(&seed)), zm = zlo + 0.5 * d;
            double T = tsfc - 0.0065 * zm; if (T < 210.0) T = 210.0;
            const double ptop = pk * exp(-9.81 * d / (287.058 * T)), pm = sqrt(pk * ptop);
            const double es = 610.78 * exp(17.269 * (T - 273.16) / (T - 35.86));
            const double qs = 0.622 * es / (pm - es > 1.0 ? pm - es : 1.0);
            const double rh = rh0 * (zm < 1500.0 ? 1.0 : exp(-(zm - 1500.0) / H));
            double q = rh * qs; if (q < 1e-7) q = 1e-7;
            double s = zlo / 12000.0; if (s > 1.0) s = 1.0;
            dz[a] = (float)d; p[a] = (float)pm; pint[a] = (float)pk; t[a] = (float)T; qv[a] = (float)q;
            pi[a] = (float)pow(pm / 1e5, 287.058 / 1012.0); rho[a] = (float)(pm / (287.058 * T));
            w[a] = (float)(wamp * sin(3.14159265 * s));
            u[a] = (float)(3.0 + sh * zm * cos(zm / 3000.0)); v[a] = (float)(-2.0 + 0.5 * sh * zm * sin(zm / 2500.0));
            qc[a] = frand(&seed) < 0.2 ? (float)(3e-4 * frand(&seed)) : 0.0f;
            qi[a] = frand(&seed) < 0.1 ? (float)(1e-4 * frand(&seed)) : 0.0f;
            pk = ptop; zlo += d;
        }
    }
    for (int call = 0; call < 2; call++) {
        const float dt = call ? 120.0f : 60.0f, dx = nz % 2 ? 900.0f : 4000.0f;
        for (int j = 0; j < ny; j++) {
            int kbmax = 0, kbm = 0, kmax = 0;
            for (int i = 0; i < nx; i++) {
                const size_t a = IX(i,0,j);
                const NsasIn in = { t + a, qv + a, qc + a, qi + a, pi + a, rho + a, w + a, dz + a, p + a, pint + a, u + a, v + a, (size_t)nx };
                int x, y, z;
                nsas_row_limits(in, n, &x, &y, &z);
                if (x > kbmax) kbmax = x;
                if (y > kbm) kbm = y;
                if (z > kmax) kmax = z;
            }
            kbmax = kbmax < n ? kbmax : n; kbm = kbm < n ? kbm : n; kmax = kmax < n ? kmax : n;
            for (int i = 0; i < nx; i++) {
                const size_t a = IX(i,0,j), c2 = (size_t)j * nx + i;
                const NsasIn in = { t + a, qv + a, qc + a, qi + a, pi + a, rho + a, w + a, dz + a, p + a, pint + a, u + a, v + a, (size_t)nx };
                NsasOut o;
                float *ws = NULL; const size_t stride = 1, nl = 0;
                (void)ws; (void)stride; (void)nl;
                for (int m = 0; m < NSAS_NARR; m++) for (int k = 0; k < (m == NSAS_ZI ? n + 1 : n); k++) memcpy(&g_arr[m][k], &fill, 4);
                nsas_setup(in, n, ws, stride, nl);
                nsas_deep(in, n, kbmax, kbm, kmax, xland[c2], dt, dx, dx <= 1000.f ? 1 : 2, ws, stride, nl, &o, NULL);
                deep += o.icps;
                nsas_shallow(in, n, xland[c2], hpbl[c2], hfx[c2], qfx[c2], dt, ws, stride, nl, &o, NULL);
                shallow += o.icps == 0 && o.ktop > 0;
                nsas_finish(in, n, dt, ws, stride, nl, &o, tth + a, tqv + a, tqc + a, tqi + a, rain + c2, prate + c2, hbot + c2, htop + c2);
            }
        }
        for (size_t a = 0; a < n3; a++) {
            if (a % ((size_t)nx * nz) / nx >= (size_t)n) continue;                /* level nz is not the scheme's */
            if (!(tth[a] == tth[a]) || !(tqv[a] == tqv[a]) || !(tqc[a] == tqc[a]) || !(tqi[a] == tqi[a])) bad = 1;
            *sum += (double)tth[a] + 1e3 * tqv[a] + 1e3 * tqc[a] + 1e3 * tqi[a];
            const float d = dt;                                                   /* carry: every fraction 1 */
            qv[a] = qv[a] + tqv[a] * d; qc[a] = qc[a] + tqc[a] * d; qi[a] = qi[a] + tqi[a] * d; t[a] = t[a] + tth[a] * pi[a] * d;
        }
        for (size_t c = 0; c < n2; c++) { if (!(rain[c] == rain[c]) || !(prate[c] == prate[c])) bad = 1; *sum += rain[c] + hbot[c] + htop[c]; }
    }
    printf("%d scheme levels: %d deep and %d shallow columns over two calls%s\n", n, deep, shallow, bad ? "  NaN!" : "");
    for (int a = 0; a < NSAS_NARR; a++) free(g_arr[a]);
    free(t); free(qv); free(qc); free(qi); free(pi); free(rho); free(w); free(dz); free(p); free(pint); free(u); free(v); free(tth); free(tqv);
    free(tqc); free(tqi); free(xland); free(hfx); free(qfx); free(hpbl); free(rain); free(prate); free(hbot); free(htop);
    return bad;
}

int main(int argc, char **argv)
{
    double sum = 0;
    if (argc > 1) {
        const int n = atoi(argv[1]);
        const int bad = run(n + 1, &sum);
        printf("%d scheme levels: %s, checksum %.17g\n", n, bad ? "NaN" : "no finding, no NaN", sum);
        return bad;
    }
    int bad = 0;
    for (int nz = NSAS_MIN_LEVELS + 1; nz <= 129; nz++) /* model levels */ bad |= run(nz, &sum);
    if (!bad) printf("scheme levels %d..128: no finding, no NaN, checksum %.17g\n", NSAS_MIN_LEVELS, sum);
    return bad;
}

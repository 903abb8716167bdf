/* tests/support/nsas_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of cu_nsas (src/physics/cu_nsas.f90:8-308, with nsas2d and
 * nscv2d) as src/physics/cu_driver.f90:354-417 calls it.  The column code is the product's own header, icar_amd/csrc/nsas_column.h,
 * compiled here for the host with gcc -O2 -ffp-contract=off against the host's libm; tests/test_nsas_oracle.py holds it bit for bit
 * to the compiled reference's vectors (tests/golden/cu_nsas_*.npz, made by tests/golden/make_golden_nsas.py).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j), the 2-D ones (ny, nx); its..kte are 1-based inclusive like the reference's;
 * the memory extents ims:ime, kms:kme, jms:jme are 1:nx, 1:nz, 1:ny and kts is 1. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#define NSAS_EXPF expf
#define NSAS_POWF powf
#define NSAS_SQRTF sqrtf
#define NSAS_DIAG
#include "../../icar_amd/csrc/nsas_column.h"

#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))

int nsas_oracle_min_levels(void) { return NSAS_MIN_LEVELS; }
int nsas_oracle_max_levels(void) { return NSAS_MAX_LEVELS; }
int nsas_oracle_workspace_arrays(void) { return NSAS_NARR; }

static NsasIn nsas_in(int nx, int nz, int i, int j, const float *t, const float *qv, const float *qc, const float *qi, const float *pi,
                      const float *rho, const float *w, const float *dz, const float *p, const float *pint, const float *u, const float *v)
{
    const size_t a = IX(i,0,j);
    NsasIn in = { t + a, qv + a, qc + a, qi + a, pi + a, rho + a, w + a, dz + a, p + a, pint + a, u + a, v + a, (size_t)nx };
    return in;
}

/* call cu_nsas(...) on its..ite, jts..jte, levels 1..kte-1 (w and pint are read up to level kte).  The four tendencies, RAINCV, PRATEC,
 * HBOT and HTOP are written on those columns only.  diag (may be NULL): (ny, nx) ints, the flags of nsas_column.h.  limits (may be
 * NULL): (ny, 3) ints, the row's kbmax, kbm, kmax; own (may be NULL): (ny, nx, 3) ints, each column's own.  fill: the bit pattern the
 * column workspace holds before each column (two different ones must give the same results).  `check` = 0 runs without the refusal of
 * the level count (the bounds program).  Returns 1 when the level count is refused. */
int nsas_oracle_run(int nx, int nz, int ny, int its, int ite, int jts, int jte, int kte, float dt, float dx, const float *t, const float *qv,
                    const float *qc, const float *qi, const float *pi, const float *rho, const float *w, const float *dz, const float *p,
                    const float *pint, const float *u, const float *v, const float *xland, const float *hpbl, const float *hfx,
                    const float *qfx, float *tend_th, float *tend_qv, float *tend_qc, float *tend_qi, float *raincv, float *pratec,
                    float *hbot, float *htop, int *diag, int *limits, int *own, unsigned fill, int check)
{
    const int n = kte - 1;
    if (check && (n < NSAS_MIN_LEVELS || n > NSAS_MAX_LEVELS || kte > nz)) return 1;
    const size_t nl = (size_t)n + 2, nw = NSAS_NARR * nl;
    float *ws = (float *)malloc(sizeof(float) * nw);
    if (!ws) return 1;
    const int dxf = dx <= 1000.f ? 1 : 2;                                           /* cu_driver.f90:357-361 */
    for (int j = jts - 1; j < jte; j++) {
        int kbmax = 0, kbm = 0, kmax = 0;
        for (int i = its - 1; i < ite; i++) {
            int a, b, c;
            nsas_row_limits(nsas_in(nx, nz, i, j, t, qv, qc, qi, pi, rho, w, dz, p, pint, u, v), n, &a, &b, &c);
            if (own) { int *o3 = own + ((size_t)j * nx + i) * 3; o3[0] = a < n ? a : n; o3[1] = b < n ? b : n; o3[2] = c < n ? c : n; }
            if (a > kbmax) kbmax = a;
            if (b > kbm) kbm = b;
            if (c > kmax) kmax = c;
        }
        kbmax = kbmax < n ? kbmax : n; kmax = kmax < n ? kmax : n; kbm = kbm < n ? kbm : n;
        if (limits) { limits[3 * j] = kbmax; limits[3 * j + 1] = kbm; limits[3 * j + 2] = kmax; }
        for (int i = its - 1; i < ite; i++) {
            const size_t a = IX(i,0,j), c2 = (size_t)j * nx + i;
            const NsasIn in = nsas_in(nx, nz, i, j, t, qv, qc, qi, pi, rho, w, dz, p, pint, u, v);
            NsasOut o;
            int dg = 0;
            for (size_t m = 0; m < nw; m++) memcpy(ws + m, &fill, sizeof(float));
            nsas_setup(in, n, ws, 1, nl);
            nsas_deep(in, n, kbmax, kbm, kmax, xland[c2], dt * 1.f, dx, dxf, ws, 1, nl, &o, &dg);
            nsas_shallow(in, n, xland[c2], hpbl[c2], hfx[c2], qfx[c2], dt * 1.f, ws, 1, nl, &o, &dg);
            nsas_finish(in, n, dt, ws, 1, nl, &o, tend_th + a, tend_qv + a, tend_qc + a, tend_qi + a, raincv + c2, pratec + c2, hbot + c2,
                        htop + c2);
            if (diag) diag[c2] = dg;
        }
    }
    free(ws);
    return 0;
}

/* tests/support/pbl_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of the simple boundary-layer scheme,
 * src/physics/pbl_simple.f90:69-291 (simple_pbl, pbl_diffusion, diffuse_variable and the four calc_* helpers), in REAL(4) with the
 * reference's operation order.  Compiled with gcc -O2 -ffp-contract=off against the host's libm (expf, sqrtf) it is bit-identical
 * to the compiled reference (tests/test_pbl_oracle.py holds it to tests/golden/pbl_simple_*.npz).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j); its..kte are 1-based inclusive like the reference's.
 * nsub_out (may be NULL): the sub-step count of every processed row.  flags (may be NULL, one int per cell, written at the half
 * levels processed): which clip / branch the coefficient of that half level took (PBL_F_* below). */
#include <math.h>
#include <stdlib.h>
#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))
enum { PBL_F_SHEAR_FLOOR = 1, PBL_F_RIG_FLOOR = 2, PBL_F_RIG_POS = 4, PBL_F_RIG_NONPOS = 8, PBL_F_PR_UPPER = 16, PBL_F_PR_LOWER = 32,
       PBL_F_KQ_UPPER = 64, PBL_F_KQ_LOWER = 128, PBL_F_DZ_CAP = 256, PBL_F_WATER = 512, PBL_F_CELL = 1024 };

int pbl_oracle_simple(int nx, int nz, int ny, float *th, float *qv, float *qc, float *qi, float *qr, float *qs, const float *um,
                      const float *vm, const float *pii, const float *rho, const float *z, const float *dz, const float *terrain,
                      const int *land, int its, int ite, int jts, int jte, int kts, int kte_in, float dt, int *nsub_out, int *flags)
{
    int kte = kte_in < nz - 1 ? kte_in : nz - 1;                                  /* :92 */
    if (kte < kts) return 1;                                                      /* maxval of nothing (:194) */
    float *Kq = malloc(sizeof(float) * nx * nz);
    float *f = malloc(sizeof(float) * nx * nz);
    float *vars[6] = {qv, th, qc, qi, qs, qr};                                    /* :196-209 */
    for (int j = jts - 1; j < jte; j++) {
        for (int k = kts - 1; k < kte; k++) for (int i = its - 1; i < ite; i++) {
            size_t a = IX(i,k,j), b = IX(i,k+1,j);
            int fl = PBL_F_CELL;
            float du = um[b] - um[a], dv = vm[b] - vm[a];
            float dzm = (dz[a] + dz[b]) * 0.5f;
            float shear = sqrtf(du*du + dv*dv) / dzm;                             /* :219-223 */
            if (shear < 1e-5f) { shear = 1e-5f; fl |= PBL_F_SHEAR_FLOOR; }
            float v1 = th[a] * (1.0f + 0.61f * qv[a] - (qc[a] + qi[a] + qr[a] + qs[a]));   /* :241-246 */
            float v2 = th[b] * (1.0f + 0.61f * qv[b] - (qc[b] + qi[b] + qr[b] + qs[b]));
            float grad = (v2 - v1) / dzm;
            float T = (th[a] * pii[a] + th[b] * pii[b]) / 2.0f;                   /* :286-289 */
            float rig = 9.81f / T * grad * 1.0f / (shear * shear);
            if (rig < -100.0f) { rig = -100.0f; fl |= PBL_F_RIG_FLOOR; }
            float stab = 0.f;                                                     /* :255-269 */
            if (rig > 0) { stab = expf(-8.5f * rig) + 0.15f / (rig + 3.0f); fl |= PBL_F_RIG_POS; }
            if (rig <= 0) { stab = 1.0f / sqrtf(1.0f - 1.6f * rig); fl |= PBL_F_RIG_NONPOS; }
            float pr = 1.5f + 3.08f * rig;
            if (pr > 4.0f) { pr = 4.0f; fl |= PBL_F_PR_UPPER; } else if (pr < 0.25f) { pr = 0.25f; fl |= PBL_F_PR_LOWER; }
            float l = 1.0f / (1.0f / (0.41f * (z[a] - terrain[(size_t)j*nx + i])) + (1.0f/250.0f));   /* :108 */
            float K = l * l * stab * shear;                                       /* :113 */
            float kq = K / pr;                                                    /* :116 */
            kq = kq * dt / ((dz[a] + dz[b]) / 2.0f);                              /* :118 */
            if (kq > 1000.f) { kq = 1000.f; fl |= PBL_F_KQ_UPPER; } else if (kq < 1.f) { kq = 1.f; fl |= PBL_F_KQ_LOWER; }
            if (land && land[(size_t)j*nx + i] == 2) { kq = kq / 1000.0f; fl |= PBL_F_WATER; }   /* :127 kLC_WATER */
            kq = kq / 2.0f;                                                       /* :131 */
            if (kq > 10.0f * dz[a]) { kq = dz[a] * 10.0f; fl |= PBL_F_DZ_CAP; }   /* :191-192 */
            Kq[k*nx + i] = kq;
            if (flags) flags[a] = fl;
        }
        float mx = -INFINITY;
        for (int k = kts - 1; k < kte; k++) for (int i = its - 1; i < ite; i++) {
            float r = Kq[k*nx+i] / dz[IX(i,k,j)];
            if (r > mx) mx = r;
        }
        int nsub = (int)ceilf(2.0f * mx);                                         /* :194 */
        if (nsub_out) nsub_out[j] = nsub;
        for (int k = kts - 1; k < kte; k++) for (int i = its - 1; i < ite; i++) Kq[k*nx+i] = Kq[k*nx+i] / (float)nsub;   /* :195 */
        for (int t = 0; t < nsub; t++) for (int v = 0; v < 6; v++) {
            float *q = vars[v];
            for (int k = kts - 1; k < kte; k++) for (int i = its - 1; i < ite; i++) {     /* :151-155 */
                size_t a = IX(i,k,j), b = IX(i,k+1,j);
                float rm = (rho[a] + rho[b]) / 2.0f;
                f[k*nx+i] = Kq[k*nx+i] * rm * (q[a] - q[b]);
            }
            for (int i = its - 1; i < ite; i++) {                                 /* :157-161 */
                int k0 = kts - 1;
                size_t a = IX(i,k0,j);
                q[a] = q[a] - f[k0*nx+i] / (dz[a] * rho[a]);
                for (int k = k0 + 1; k < kte; k++) { a = IX(i,k,j); q[a] = q[a] - (f[k*nx+i] - f[(k-1)*nx+i]) / (dz[a] * rho[a]); }
                a = IX(i,kte,j); size_t c = IX(i,kte-1,j);
                q[a] = q[a] + f[(kte-1)*nx+i] / (dz[c] * rho[c]);
            }
        }
    }
    free(Kq); free(f);
    return 0;
}

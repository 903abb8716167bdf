/* tests/support/sfc_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of the surface-flux slot as it runs for landsurface = kLSM_BASIC
 * with watersurface 0, 1 or kWATER_SIMPLE: the 10 m diagnostics of diagnostic_update (src/main/time_step.f90:143-161), the gated
 * block of lsm (src/physics/lsm_driver.f90:1028-1073: windspd, the `where(wind==0)` of calc_exchange_coefficient :251, water_simple
 * of src/physics/water_simple.f90:18-136) and apply_fluxes (lsm_driver.f90:361-423), in REAL(4) with the reference's operation
 * order.  Compiled with gcc -O2 -ffp-contract=off against the host's libm (expf, logf) it is bit-identical to the compiled
 * reference (tests/test_sfc_oracle.py holds it to tests/golden/sfc_basic_*.npz).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j), the 2-D ones (ny, nx); its..kte are 1-based inclusive like the
 * reference's; the memory extents ims:ime, kms:kme, jms:jme are 1:nx, 1:nz, 1:ny.
 * Reproduced quirks: water_simple and the 10 m diagnostics run on 2..nx-1, 2..ny-1 of the MEMORY rectangle; apply_fluxes' level
 * search keeps the ABSOLUTE index of the last level below sfc_layer_thickness and its loop then runs kts .. kts+nz, one level more
 * (and, with kts > 1, kts-1 levels more still); the qv floor covers the whole array.  sum_mode: how sum(dz(i,kts:k-1,j)) is
 * formed -- 0 a plain REAL(4) loop, 1 Kahan in REAL(4), 2 Kahan in REAL(8) rounded once; the compiled reference settles which
 * (tests/sfc_oracle.py: SUM_MODE). */
#include <math.h>
#include <stddef.h>
#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))
enum { SF_CELL = 1, SF_WATER = 2, SF_ICE = 4, SF_CLIP = 8, SF_RI_NEG = 16, SF_USTAR_FLOOR = 32, SF_WIND0 = 64 };
enum { AF_LAYER = 1, AF_MIN1 = 2, AF_MAX0 = 4, AF_FLOOR = 8, AF_UPPER = 16 };
static const float karman = 0.41f, gravity = 9.81f, LH_vaporization = 2260000.0f, cp = 1012.0f;   /* icar_constants.f90:389-397 */
static const float SMALL_QV = 1e-10f;                                                              /* lsm_driver.f90:87 */
enum { kLC_WATER = 2 };

/* time_step.f90:143-161 on ims+1:ime-1, jms+1:jme-1 */
void sfc_oracle_diag_10m(int nx, int nz, int ny, const float *z, const float *terrain, const float *z0, const float *u_mass,
                         const float *v_mass, float *u10, float *v10, float *ustar)
{
    for (int j = 1; j < ny - 1; j++) for (int i = 1; i < nx - 1; i++) {
        size_t c2 = (size_t)j * nx + i, a = IX(i,0,j);
        float currw = karman / logf((z[a] - terrain[c2]) / z0[c2]);
        float lastw = logf(10.0f / z0[c2]) / karman;
        float t = u_mass[a] * currw;
        u10[c2] = t * lastw;
        t = v_mass[a] * currw;
        v10[c2] = t * lastw;
        ustar[c2] = sqrtf(u_mass[a] * u_mass[a] + v_mass[a] * v_mass[a]) * currw;
    }
}

static float sat_mr(float t, float p, int *fl)                       /* water_simple.f90:18-55 */
{
    float a, b;
    if (t < 273.15f) { a = 21.8745584f; b = 7.66f; *fl |= SF_ICE; } else { a = 17.2693882f; b = 35.86f; }
    float e_s = 610.78f * expf(a * (t - 273.16f) / (t - b));
    if ((p - e_s) <= 0) { e_s = p * 0.99999f; *fl |= SF_CLIP; }
    return 0.6219907f * e_s / (p - e_s);
}

/* lsm_driver.f90:1028-1073 with watersurface = kWATER_SIMPLE; windspd (ny, nx) is the module array, written whole */
void sfc_oracle_water_simple(int nx, int nz, int ny, const float *u10, const float *v10, const float *sst, const float *psfc,
                             const float *ustar, const float *qv, const float *temperature, const float *z, const float *terrain,
                             const int *landmask, float *sensible, float *latent, float *z0, float *qsfc, float *qfx, float *tskin,
                             float *windspd, int run_water, int *flags)
{
    const float k75 = 75 * (karman * karman);                        /* 75*karman**2, folded */
    for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
        size_t c2 = (size_t)j * nx + i;
        int fl = 0;
        float w = sqrtf(u10[c2] * u10[c2] + v10[c2] * v10[c2]);     /* :1028 */
        if (w == 0) { w = 1e-5f; fl |= SF_WIND0; }                   /* :251 */
        windspd[c2] = w;
        if (flags) flags[c2] = fl;
    }
    if (!run_water) return;
    for (int j = 1; j < ny - 1; j++) for (int i = 1; i < nx - 1; i++) {
        size_t c2 = (size_t)j * nx + i, a = IX(i,0,j);
        int fl = (flags ? flags[c2] : 0) | SF_CELL;
        if (landmask[c2] == kLC_WATER) {
            fl |= SF_WATER;
            qsfc[c2] = 0.98f * sat_mr(sst[c2], psfc[c2], &fl);
            if (ustar[c2] < 1e-7f) fl |= SF_USTAR_FLOOR;
            z0[c2] = 8e-6f / fmaxf(ustar[c2], 1e-7f);
            float zz = z[a] - terrain[c2];                           /* z_atm of lsm_init :992 */
            float r = (zz + z0[c2]) / z0[c2];
            float lnz = logf(r);
            float base = (k75 * sqrtf(r)) / (lnz * lnz);
            float q = karman / lnz;
            lnz = q * q;
            float wind = windspd[c2], airt = temperature[a], tsk = sst[c2];
            float Ri = gravity / airt * (airt - tsk) * zz / (wind * wind);
            float C;
            if (Ri < 0) { C = lnz * (1.0f - (15.0f * Ri) / (1.0f + (base * sqrtf((-1.0f) * Ri)))); fl |= SF_RI_NEG; }
            else C = lnz * 1.0f / ((1.0f + 15.0f * Ri) * sqrtf(1.0f + 5.0f * Ri));
            sensible[c2] = C * wind * (tsk - airt);
            qfx[c2] = C * wind * (qsfc[c2] - qv[a]);
            latent[c2] = qfx[c2] * LH_vaporization;
            tskin[c2] = tsk;
        }
        if (flags) flags[c2] = fl;
    }
}

/* apply_fluxes :370-376: the last k (absolute, 1-based) at which the running sum of maxval(dz_interface(:,k,:)) is below thick; 0: none */
int sfc_oracle_layers(int nx, int nz, int ny, const float *dz, float thick, int kts, int kte)
{
    int nzl = 0;
    float lf = 0;
    for (int k = kts - 1; k < kte; k++) {
        float m = dz[IX(0,k,0)];
        for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) if (dz[IX(i,k,j)] > m) m = dz[IX(i,k,j)];
        lf = m + lf;
        if (lf < thick) nzl = k + 1;
    }
    return nzl;
}

static float sum_below(const float *dz, size_t a0, size_t sk, int n, int mode)
{
    if (mode == 0) { float s = 0; for (int m = 0; m < n; m++) s = s + dz[a0 + m * sk]; return s; }
    if (mode == 1) {
        float s = 0, c = 0;
        for (int m = 0; m < n; m++) { volatile float next = dz[a0 + m * sk] - c; volatile float old = s; s = old + next; volatile float d = s - old; c = d - next; }
        return s;
    }
    double s = 0, c = 0;
    for (int m = 0; m < n; m++) { volatile double next = (double)dz[a0 + m * sk] - c; volatile double old = s; s = old + next; volatile double d = s - old; c = d - next; }
    return (float)s;
}

/* apply_fluxes :378-419.  Returns 1 where the reference would read past kte (kts + nzl > kte).  flags (ny, nz, nx) or NULL */
int sfc_oracle_apply_fluxes(int nx, int nz, int ny, float *th, float *qv, const float *density, const float *pii, const float *dz,
                            const float *sensible, const float *latent, float dt, float sh_frac, float lh_frac, float thick, int nzl,
                            int its, int ite, int jts, int jte, int kts, int kte, int sum_mode, int *flags)
{
    if (kts + nzl > kte) return 1;
    if (flags) for (size_t t = 0; t < (size_t)nx * nz * ny; t++) flags[t] = 0;
    for (int j = jts - 1; j < jte; j++) for (int k = kts - 1; k <= kts - 1 + nzl; k++) for (int i = its - 1; i < ite; i++) {
        size_t a = IX(i,k,j), c2 = (size_t)j * nx + i;
        int fl = AF_LAYER;
        float lf;
        if (k == kts - 1) lf = fminf(1.0f, thick / dz[a]);
        else {
            fl |= AF_UPPER;
            lf = (thick - sum_below(dz, IX(i,kts-1,j), nx, k - (kts - 1), sum_mode)) / dz[a];
            if (!(lf < 1.0f)) { lf = 1.0f; fl |= AF_MIN1; }
            if (!(lf > 0.0f)) { lf = 0.0f; fl |= AF_MAX0; }
        }
        float dTemp = (sh_frac * sensible[c2] * dt / cp) / (density[a] * thick);
        th[a] = th[a] + (dTemp / pii[a]) * lf;
        float lhdQV = (lh_frac * latent[c2] / LH_vaporization * dt) / (density[a] * thick);
        qv[a] = qv[a] + lhdQV * lf;
        if (flags) flags[a] = fl;
    }
    for (size_t t = 0; t < (size_t)nx * nz * ny; t++) if (qv[t] < SMALL_QV) { qv[t] = SMALL_QV; if (flags) flags[t] |= AF_FLOOR; }
    return 0;
}

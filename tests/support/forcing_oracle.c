/* tests/support/forcing_oracle.c -- TEST INFRASTRUCTURE: the CPU restatement of the forcing update.  The arithmetic is the product's
 * own header icar_amd/csrc/forcing_interp.h compiled for the host (gcc -O2 -ffp-contract=off, the C library's expf / powf); this file
 * only loops over the cells.  smooth_array is oracle/wind_oracle.c's (orc_smooth_array_ydim3), called from tests/forcing_oracle.py.
 * With -DFI_CONTRACT=1 the product-sums are FMAs: tests/golden/make_golden_forcing.py builds that form too, to show that the compiled
 * reference does not contract. */
#include <math.h>
#include <stddef.h>
#define FI_EXPF expf
#define FI_POWF powf
#include "../../icar_amd/csrc/forcing_interp.h"

int fo_contract(void) { return FI_CONTRACT; }

/* geo_interp + vinterp (interpolate_variable with vert_interp): lo(nx_f, nz_f, ny_f) -> out(nx, nz, ny) */
void fo_geo_vinterp(const float *lo, int nx_f, int nz_f, int ny_f, const int *gx, const int *gy, const float *gw, const int *vz,
                    const float *vw, int nx, int nz, int ny, float *out)
{
    (void)ny_f;
    for (int j = 0; j < ny; ++j)
        for (int k = 0; k < nz; ++k)
            for (int i = 0; i < nx; ++i) {
                const size_t c = 4 * ((size_t)i + (size_t)nx * j), v = 2 * ((size_t)i + (size_t)nx * ((size_t)k + (size_t)nz * j));
                int c4[4];
                for (int l = 0; l < 4; ++l) c4[l] = fi_corner(gx[c + l], gy[c + l], nx_f, nz_f);
                const float a = fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, vz[v]);
                const float b = fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, vz[v + 1]);
                out[(size_t)i + (size_t)nx * ((size_t)k + (size_t)nz * j)] = fi_vinterp(a, vw[v], b, vw[v + 1]);
            }
}

/* geo_interp and the vert_interp = .false. branch: level k of the output is level min(k, nz_f) of temp_3d */
void fo_geo_novert(const float *lo, int nx_f, int nz_f, int ny_f, const int *gx, const int *gy, const float *gw, int nx, int nz, int ny,
                   float *out)
{
    (void)ny_f;
    for (int j = 0; j < ny; ++j)
        for (int k = 0; k < nz; ++k)
            for (int i = 0; i < nx; ++i) {
                const size_t c = 4 * ((size_t)i + (size_t)nx * j);
                int c4[4];
                for (int l = 0; l < 4; ++l) c4[l] = fi_corner(gx[c + l], gy[c + l], nx_f, nz_f);
                out[(size_t)i + (size_t)nx * ((size_t)k + (size_t)nz * j)] = fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, k + 1);
            }
}

/* adjust_pressure: p_in, th_in, z_out, p_out (nx, nz, ny); z_in (nx, nz_f, ny) with nz_f >= nz; diag (nx, nz, ny) or NULL */
void fo_adjust_pressure(const float *p_in, const float *th_in, const float *z_in, const float *z_out, float *p_out, int nx, int nz,
                        int nz_f, int ny, unsigned char *diag)
{
    /* the columns of z_in have another row pitch than the others: gather each into a column of the model's pitch */
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            float zc[1024];
            for (int k = 0; k < nz && k < 1024; ++k) zc[k] = z_in[(size_t)i + (size_t)nx * ((size_t)k + (size_t)nz_f * j)];
            const size_t o = (size_t)i + (size_t)nx * (size_t)nz * j;
            float pc[1024], tc[1024], oc[1024], rc[1024]; unsigned char dc[1024];
            for (int k = 0; k < nz && k < 1024; ++k) { pc[k] = p_in[o + (size_t)nx * k]; tc[k] = th_in[o + (size_t)nx * k]; oc[k] = z_out[o + (size_t)nx * k]; }
            fi_adjust_pressure_column(pc, tc, zc, oc, rc, nz, 1, diag ? dc : NULL);
            for (int k = 0; k < nz && k < 1024; ++k) { p_out[o + (size_t)nx * k] = rc[k]; if (diag) diag[o + (size_t)nx * k] = dc[k]; }
        }
}

void fo_delta(float *dqdt, const float *data, size_t n, double dt_seconds)
{
    for (size_t t = 0; t < n; ++t) dqdt[t] = fi_delta(dqdt[t], data[t], dt_seconds);
}

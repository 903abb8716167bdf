/* tests/support/forcing_bounds_main.c -- TEST INFRASTRUCTURE: a stand-alone program around icar_amd/csrc/forcing_interp.h, built with the
 * address and undefined-behaviour sanitizers by tests/test_forcing_bounds.py and run on its own.  Every model level count 1..66 against
 * every forcing level count 2..20, every array an allocation of exactly the reference's extent (so that one element read or written past
 * it is reported): geo_interp + vinterp, the vert_interp = .false. branch, and adjust_pressure wherever the forcing has at least the
 * model's levels.  Where it has fewer the REFERENCE reads out of bounds -- adjust_pressure indexes input_z(i, min(nz, in_z_idx + 1), j)
 * with the model's nz although input_z has nz_f levels (domain_obj.f90:2680-2690; the pressure and the potential temperature it indexes
 * the same way have been padded to nz levels, :2752-2760, and are not the problem) -- and icar_hip_forcing_configure refuses those
 * combinations; the program counts them and does not run them.
 * Prints "forcing_bounds: R run, S refused" and returns 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#define FI_EXPF expf
#define FI_POWF powf
#include "../../icar_amd/csrc/forcing_interp.h"

static unsigned rnd_state = 12345u;
static unsigned rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static float frnd(void) { return (float)(rnd() % 100000) / 100000.0f; }

int main(void)
{
    const int nx = 5, ny = 3, nx_f = 4, ny_f = 3;
    int run = 0, refused = 0;
    for (int nz = 1; nz <= 66; ++nz)
        for (int nz_f = 2; nz_f <= 20; ++nz_f) {
            const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, nf = (size_t)nx_f * nz_f * ny_f;
            int *gx = malloc(4 * n2 * sizeof(int)), *gy = malloc(4 * n2 * sizeof(int)), *vz = malloc(2 * n3 * sizeof(int));
            float *gw = malloc(4 * n2 * sizeof(float)), *vw = malloc(2 * n3 * sizeof(float)), *lo = malloc(nf * sizeof(float)), *th = malloc(nf * sizeof(float));
            float *out = malloc(n3 * sizeof(float)), *p_nv = malloc(n3 * sizeof(float)), *th_nv = malloc(n3 * sizeof(float)), *p_out = malloc(n3 * sizeof(float));
            float *z_out = malloc(n3 * sizeof(float)), *z_in = malloc(n2 * nz_f * sizeof(float));
            for (size_t t = 0; t < 4 * n2; ++t) { gx[t] = 1 + (int)(rnd() % nx_f); gy[t] = 1 + (int)(rnd() % ny_f); gw[t] = frnd(); }
            for (size_t t = 0; t < n3; ++t) {
                const unsigned r = rnd() % 10;
                const int z1 = r == 0 ? 1 : r == 9 ? nz_f : 1 + (int)(rnd() % (nz_f - 1));
                vz[2 * t] = z1; vz[2 * t + 1] = (r == 0 || r == 9) ? z1 : z1 + 1;
                vw[2 * t] = frnd(); vw[2 * t + 1] = 1.0f - vw[2 * t];
            }
            /* the first and the last corner and level of the forcing grid are named somewhere */
            gx[0] = 1; gy[0] = 1; gx[4 * n2 - 1] = nx_f; gy[4 * n2 - 1] = ny_f; vz[0] = 1; vz[2 * n3 - 1] = nz_f;
            for (size_t t = 0; t < nf; ++t) { lo[t] = 30000.0f + 70000.0f * frnd(); th[t] = 270.0f + 60.0f * frnd(); }
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    float a = 0.0f, b = 0.0f;
                    for (int k = 0; k < nz; ++k) { a += 20.0f + 700.0f * frnd(); z_out[i + nx * (k + nz * j)] = a; }
                    for (int k = 0; k < nz_f; ++k) { b += 20.0f + 700.0f * frnd(); z_in[i + nx * (k + nz_f * j)] = b; }
                }
            for (int j = 0; j < ny; ++j)
                for (int k = 0; k < nz; ++k)
                    for (int i = 0; i < nx; ++i) {
                        const size_t c = 4 * ((size_t)i + (size_t)nx * j), o = (size_t)i + (size_t)nx * ((size_t)k + (size_t)nz * j);
                        int c4[4];
                        for (int l = 0; l < 4; ++l) c4[l] = fi_corner(gx[c + l], gy[c + l], nx_f, nz_f);
                        out[o] = fi_vinterp(fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, vz[2 * o]), vw[2 * o], fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, vz[2 * o + 1]), vw[2 * o + 1]);
                        p_nv[o] = fi_geo_cell(lo, nx_f, nz_f, c4, gw + c, k + 1);
                        th_nv[o] = fi_geo_cell(th, nx_f, nz_f, c4, gw + c, k + 1);
                    }
            if (nz_f >= nz) {
                for (int j = 0; j < ny; ++j)
                    for (int i = 0; i < nx; ++i) {
                        const size_t col = (size_t)i + (size_t)nx * nz * j;
                        fi_adjust_pressure_column(p_nv + col, th_nv + col, z_in + i + (size_t)nx * nz_f * j, z_out + col, p_out + col, nz, (size_t)nx, NULL);
                    }
                for (size_t t = 0; t < n3; ++t) if (!(p_out[t] > 0.0f) || !isfinite(out[t])) { printf("forcing_bounds: bad value at nz %d nz_f %d\n", nz, nz_f); return 1; }
                ++run;
            } else
                ++refused;
            free(gx); free(gy); free(vz); free(gw); free(vw); free(lo); free(th); free(out); free(p_nv); free(th_nv); free(p_out); free(z_out); free(z_in);
        }
    printf("forcing_bounds: %d run, %d refused\n", run, refused);
    return 0;
}

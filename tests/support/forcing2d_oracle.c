/* tests/support/forcing2d_oracle.c -- TEST INFRASTRUCTURE: the CPU restatement of the 2-D forced variables.  The arithmetic is the
 * product's own header icar_amd/csrc/forcing2d_cell.h compiled for the host (gcc -O2 -ffp-contract=off); this file only loops over the
 * cells.  With -DF2_CONTRACT=1 the product-sums are FMAs: tests/golden/make_golden_forcing2d.py builds that form too, to show that the
 * compiled reference does not contract. */
#include <stddef.h>
#include "../../icar_amd/csrc/forcing2d_cell.h"

int f2o_contract(void) { return F2_CONTRACT; }

/* geo_interp2d: lo(nx_f, ny_f) -> out(nx, ny) through geolut x, y, w (4, nx, ny) */
void f2o_geo_interp2d(const float *lo, int nx_f, int ny_f, const int *gx, const int *gy, const float *gw, int nx, int ny, float *out)
{
    (void)ny_f;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const size_t c = (size_t)i + (size_t)nx * j;
            out[c] = f2_geo_cell(lo, nx_f, gx + 4 * c, gy + 4 * c, gw + 4 * c);
        }
}

void f2o_delta(float *dqdt, const float *data, size_t n, double dt_seconds)
{
    for (size_t t = 0; t < n; ++t) dqdt[t] = f2_delta(dqdt[t], data[t], dt_seconds);
}

void f2o_apply(float *x, const float *dqdt, size_t n, double dt_seconds)
{
    for (size_t t = 0; t < n; ++t) x[t] = f2_apply(x[t], dqdt[t], dt_seconds);
}

void f2o_precip(double *accumulated, const float *external, size_t n, double dt_seconds)
{
    for (size_t t = 0; t < n; ++t) accumulated[t] = f2_precip(accumulated[t], external[t], dt_seconds);
}

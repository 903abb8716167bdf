// icar_amd/csrc/forcing2d_cell.h -- the per-cell arithmetic of the 2-D forced variables (sst, shortwave, longwave,
// external_precipitation), for the device (forcing2d.hip) and for the host (tests/support/forcing2d_oracle.c compiles this very file
// with a C compiler).
//
// Reference algorithm (src/...):
//   geo_interp2d           utilities/geo_reader.f90:1142-1182   the triangular interpolation of a 2-D forcing array
//   update_delta_fields    objects/domain_obj.f90:2355-2356     dqdt_2d = (dqdt_2d - data_2d) / dt%seconds()
//   apply_forcing          objects/domain_obj.f90:2400-2402     data_2d = data_2d + (dqdt_2d * dt%seconds())
//                          objects/domain_obj.f90:2442-2444     accumulated_precipitation%data_2dd += external_precipitation%data_2d * dt
// REAL(4) in the reference's operation order, REAL(8) where dt%seconds() enters.  The compiled reference (flang -O2) contracts none of
// the product-sums below into an FMA: tests/golden/make_golden_forcing2d.py evaluates both forms (F2_CONTRACT) and refuses to write
// vectors unless exactly the plain one reproduces the reference bit for bit.
//
// All arrays are in Fortran order, i fastest: a forcing array lo(nx_f, ny_f), the look-up tables x, y, w(4, nx, ny) exactly as geo_LUT
// leaves them (1-based indices into the forcing array).
#pragma once

#ifndef F2_FN
#define F2_FN static inline
#endif
#ifndef F2_CONTRACT
#define F2_CONTRACT 0
#endif
#if F2_CONTRACT
#define F2_MULADD(a, b, c) __builtin_fmaf((a), (b), (c))
#define F2_MULADD_D(a, b, c) __builtin_fma((a), (b), (c))
#else
#define F2_MULADD(a, b, c) ((c) + (a) * (b))
#define F2_MULADD_D(a, b, c) ((c) + ((a) * (b)))
#endif

/* geo_interp2d (:1165-1181) for one output cell: lo is the forcing array (nx_f columns), x4 / y4 the cell's four corners (1-based) and
 * w4 their weights (w4[3] is never read).  The output starts at 0 (so does local_center): a sum of negative zeros is +0. */
F2_FN float f2_geo_cell(const float *lo, int nx_f, const int *x4, const int *y4, const float *w4)
{
    float out = 0.0f, center = 0.0f;
    for (int l = 0; l < 4; ++l) {
        const float v = lo[(x4[l] - 1) + nx_f * (y4[l] - 1)];     /* a forcing array has fewer than 2^31 elements */
        center = center + v;
        if (l < 2) out = F2_MULADD(v, w4[l], out);
    }
    return F2_MULADD(center / 4.0f, w4[2], out);
}

/* update_delta_fields (:2356): the difference in REAL(4), the quotient by the REAL(8) dt%seconds() in double, rounded once */
F2_FN float f2_delta(float dqdt, float data, double dt_seconds) { return (float)((double)(dqdt - data) / dt_seconds); }

/* apply_forcing (:2402): REAL + REAL * REAL(8), evaluated in REAL(8), rounded once on assignment */
F2_FN float f2_apply(float x, float dqdt, double dt_seconds) { return (float)F2_MULADD_D((double)dqdt, dt_seconds, (double)x); }

/* apply_forcing (:2443): the REAL(8) accumulated precipitation takes the forced rate times dt%seconds() */
F2_FN double f2_precip(double accumulated, float external, double dt_seconds) { return F2_MULADD_D((double)external, dt_seconds, accumulated); }

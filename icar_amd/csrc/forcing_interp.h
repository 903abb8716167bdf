// icar_amd/csrc/forcing_interp.h -- the per-cell and per-column arithmetic of the forcing update, for the device (forcing.hip) and
// for the host (tests/support/forcing_oracle.c compiles this very file with a C compiler).
//
// Reference algorithm (src/...):
//   geo_interp             utilities/geo_reader.f90:1069-1136   the triangular interpolation from the forcing grid
//   vinterp, axis 2        utilities/vinterp.f90:284-295        lo(z1) w1 + lo(z2) w2
//   interpolate_variable   objects/domain_obj.f90:2709-2809     vert_interp = .false. (:2750-2760): the first nz levels, the forcing's
//                                                               top level repeated where it has fewer
//   adjust_pressure        objects/domain_obj.f90:2656-2702     the findz walk, temp_t = exner_function(p) theta
//   update_pressure        utilities/atm_utilities.f90:611-653  lowresT present, hiresT absent
//   update_delta_fields    objects/domain_obj.f90:2339-2372     (dqdt - data) / dt%seconds()
// REAL(4) in the reference's operation order.  The compiled reference (flang -O2) contracts none of the product-sums below into an
// FMA: tests/golden/make_golden_forcing.py evaluates both forms (FI_CONTRACT) and refuses to write vectors unless exactly the plain
// one reproduces the reference bit for bit.  exp and the real-exponent power are the C library's (the includer names them: FI_EXPF,
// FI_POWF).
//
// All arrays are in Fortran order, i fastest: a forcing array lo(nx_f, nz_f, ny_f), the look-up tables x, y, w(4, nx, ny) and
// z, w(2, nx, nz, ny) exactly as geo_LUT and vLUT leave them (1-based indices into the forcing array).
#pragma once

#ifndef FI_FN
#define FI_FN static inline
#endif
#ifndef FI_CONTRACT
#define FI_CONTRACT 0
#endif
#if FI_CONTRACT
#define FI_MULADD(a, b, c) __builtin_fmaf((a), (b), (c))
#else
#define FI_MULADD(a, b, c) ((a) * (b) + (c))
#endif

/* icar_constants.f90:391-394, the PARAMETER expressions folded in REAL(4) as flang folds them */
#define FI_RD 287.058f
#define FI_CP 1012.0f
#define FI_GRAVITY 9.81f

/* what the coverage conditions of tests/test_forcing_oracle.py count (host only: a non-null diag) */
enum { FI_D_STAY1 = 1, FI_D_JUMP = 2, FI_D_EXIT = 4, FI_D_DZ_POS = 8, FI_D_DZ_NEG = 16 };

/* the element of level 1 of the forcing column (x, y), 1-based as geolut holds them; a forcing array has fewer than 2^31 elements */
FI_FN int fi_corner(int x, int y, int nx_f, int nz_f) { return (x - 1) + nx_f * nz_f * (y - 1); }

/* geo_interp (:1106-1123) for one output cell: lo is the forcing array, c4 the cell's four corners (fi_corner) and w4 their weights
 * (w4[3] is never read), level the 1-based output level, clamped to the forcing's level count as the reference clamps it.  The output
 * starts at 0 (so does local_center): a sum of negative zeros is +0. */
FI_FN float fi_geo_cell(const float *lo, int nx_f, int nz_f, const int *c4, const float *w4, int level)
{
    const int lev = nx_f * ((level < nz_f ? level : nz_f) - 1);
    float out = 0.0f, center = 0.0f;
    for (int l = 0; l < 4; ++l) {
        const float v = lo[c4[l] + lev];
        center = center + v;
        if (l < 2) out = FI_MULADD(v, w4[l], out);
    }
    return FI_MULADD(center / 4.0f, w4[2], out);
}

/* vinterp (:292): a and b are temp_3d at the two levels vert_lut names, rounded to REAL(4) where the reference stores them */
FI_FN float fi_vinterp(float a, float w1, float b, float w2)
{
#if FI_CONTRACT
    return __builtin_fmaf(a, w1, b * w2);
#else
    return a * w1 + b * w2;
#endif
}

/* exner_function (atm_utilities.f90:682-691): po = 100000 is an integer in the reference, so p / 100000. */
FI_FN float fi_exner(float p) { return FI_POWF(p / 100000.0f, FI_RD / FI_CP); }

/* adjust_pressure (:2674-2699) for one column.  p_in and th_in are the pressure and the potential temperature of the forcing on the
 * model's columns WITHOUT vertical interpolation, z_in is forcing%geo%z (its first nz levels are read: nz_f >= nz is the caller's
 * to check, the reference reads out of bounds otherwise), z_out is domain%geo%z; all four and p_out are columns with `stride`
 * elements between levels.  p_out must not alias p_in: the walk reads levels of p_in below the one it writes. */
FI_FN void fi_adjust_pressure_column(const float *p_in, const float *th_in, const float *z_in, const float *z_out, float *p_out,
                                     int nz, size_t stride, unsigned char *diag)
{
    int idx = 1;                                                  /* in_z_idx */
    for (int k = 1; k <= nz; ++k) {
        const float zo = z_out[(size_t)(k - 1) * stride];
        int moved = 0, left = 0;
        for (;;) {                                                /* findz */
            const int up = idx + 1 < nz ? idx + 1 : nz;
            if (!(zo > (z_in[(size_t)(idx - 1) * stride] + z_in[(size_t)(up - 1) * stride]) / 2.0f)) break;
            idx = up; ++moved;
            if (idx == nz) { left = 1; break; }
        }
        const float tz = z_in[(size_t)(idx - 1) * stride], tp = p_in[(size_t)(idx - 1) * stride];
        const float tt = fi_exner(tp) * th_in[(size_t)(idx - 1) * stride];
        const float dz = tz - zo;                                 /* update_pressure: z_lo - z_hi, tmean = lowresT */
        p_out[(size_t)(k - 1) * stride] = tp * FI_EXPF(((FI_GRAVITY / FI_RD) * dz) / tt);
        if (diag) diag[(size_t)(k - 1) * stride] = (unsigned char)((idx == 1 ? FI_D_STAY1 : 0) | (moved > 1 ? FI_D_JUMP : 0) | (left ? FI_D_EXIT : 0) |
                                                                   (dz > 0.0f ? FI_D_DZ_POS : 0) | (dz < 0.0f ? FI_D_DZ_NEG : 0));
    }
}

/* update_delta_fields (:2360): the difference in REAL(4), the quotient by the REAL(8) dt%seconds() in double, rounded once */
FI_FN float fi_delta(float dqdt, float data, double dt_seconds) { return (float)((double)(dqdt - data) / dt_seconds); }

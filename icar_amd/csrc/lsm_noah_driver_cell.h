// icar_amd/csrc/lsm_noah_driver_cell.h -- the statements of lsm() around the call of lsm_noah (src/physics/lsm_driver.f90 with
// landsurface = kLSM_NOAH), one cell at a time.  Compiled by hipcc for the kernels of lsm_noah_driver.hip and by gcc for the CPU
// restatement tests/support/lsm_noah_driver_oracle.c: one text, two compilers.  The includer defines
//   LND_FN     the function qualifiers
//   LND_LOGF   logf, LND_EXPF expf: glibc's, bit for bit (glibc_flt32.h on the device)
//   LND_SQRTF  the IEEE square root
// REAL(4) in the reference's operation order, to be compiled without contraction; x**2 is x*x and x**4 is ((x*x)*x)*x, which is how
// flang lowers them (tests/golden/make_golden_lsm_noah.py compares with the compiled statements).
//
// exchange_term = 1 is the only value lsm_init ever sets (:535), so calc_mahrt_holtslag_exchange_coefficient and F2_formula (:269-297)
// are unreachable and are not built.  Of surface_diagnostics (:299-359) only the bulk arm is built: lsm_var_request allocates
// temperature_2m_veg for Noah but not temperature_2m_bare (:119-129), `associated(T2bare)` is false and both outer arms are dead.
// domain%rain_fraction (:1208) is allocated only with the bias-correction options and is not built; rain_bucket (:1291) feeds a term
// that is commented out (:1207) and has no array.
#pragma once

#define LND_KARMAN 0.41f                              /* icar_constants.f90:397 */
#define LND_GRAVITY 9.81f
#define LND_RD 287.058f                               /* :391 */
#define LND_CP 1012.0f                                /* :393 */
#define LND_STEFAN_BOLTZMANN 5.67e-8f                 /* :396 */
#define LND_K75 (75 * (LND_KARMAN * LND_KARMAN))      /* 75*karman**2 as flang folds it */
#define LND_SMALL_QV 1e-10f                           /* lsm_driver.f90:87 */
#define LND_MAX_EXCHANGE_C 0.5f                       /* :88 */
#define LND_MIN_EXCHANGE_C 0.004f                     /* :89 */
#define LND_LC_LAND 1

/* mod_atm_utilities' sat_mr (atm_utilities.f90:523-560); water_simple.f90:18-55 is the same text */
LND_FN float lnd_sat_mr(float t, float p)
{
    float a, b, e_s;
    if (t < 273.15f) { a = 21.8745584f; b = 7.66f; }
    else { a = 17.2693882f; b = 35.86f; }
    e_s = 610.78f * LND_EXPF(a * (t - 273.16f) / (t - b));
    if ((p - e_s) <= 0) e_s = p * 0.99999f;
    return 0.6219907f * e_s / (p - e_s);
}

/* lnz_atm_term and base_exchange_term with exchange_term = 1 (:993-996 from Z0, :1282-1285 from the new roughness_z0) */
LND_FN void lnd_exchange_terms(float z_atm, float z0, float *lnz_atm_term, float *base_exchange_term)
{
    const float r = (z_atm + z0) / z0;
    const float lnz = LND_LOGF(r);
    const float q = LND_KARMAN / lnz;
    *base_exchange_term = (LND_K75 * LND_SQRTF(r)) / (lnz * lnz);
    *lnz_atm_term = q * q;
}

/* windspd (:1028), calc_exchange_coefficient (:244-265) and, behind water_simple, which only reads windspd,
   `where(windspd<1) windspd=1; CHS = CHS * windspd; CHS2 = CHS; CQS2 = CHS` (:1144-1147): *chs is what all three arrays receive.
   flags: 1 Ri < 0, 2 Ri >= 0, 4 clamped at the maximum, 8 at the minimum, 16 wind == 0 */
LND_FN void lnd_exchange(float u10, float v10, float tskin, float airt, float z_atm, float lnz_atm_term, float base_exchange_term,
                         float *ri, float *chs, int *flags)
{
    float wind = LND_SQRTF(u10 * u10 + v10 * v10);
    float C = 0.0f, Ri;
    int f = 0;
    if (wind == 0) { wind = 1e-5f; f |= 16; }
    Ri = LND_GRAVITY / airt * (airt - tskin) * z_atm / (wind * wind);
    if (Ri < 0) { C = lnz_atm_term * (1.0f - (15.0f * Ri) / (1.0f + (base_exchange_term * LND_SQRTF((-1.0f) * Ri)))); f |= 1; }
    if (Ri >= 0) { C = lnz_atm_term * 1.0f / ((1.0f + 15.0f * Ri) * LND_SQRTF(1.0f + 5.0f * Ri)); f |= 2; }
    if (C > LND_MAX_EXCHANGE_C) { C = LND_MAX_EXCHANGE_C; f |= 4; }
    if (C < LND_MIN_EXCHANGE_C) { C = LND_MIN_EXCHANGE_C; f |= 8; }
    if (wind < 1) wind = 1;
    *ri = Ri;
    *chs = C * wind;
    *flags = f;
}

/* :1207: a REAL(8) difference stored into a REAL(4) array */
LND_FN float lnd_current_precipitation(double accumulated_precipitation, double rainbl) { return (float)(accumulated_precipitation - rainbl); }

/* :1280 */
LND_FN float lnd_max_swe(float swe, float max_swe) { return swe > max_swe ? max_swe : swe; }

/* :1289 */
LND_FN float lnd_longwave_up(float emiss, float tskin)
{
    return LND_STEFAN_BOLTZMANN * emiss * (((tskin * tskin) * tskin) * tskin);
}

/* :1524-1527 with DZS = 0.1, 0.3, 0.6, 1.0 (allocate_noah_data) */
LND_FN float lnd_soil_totalmoisture(float s1, float s2, float s3, float s4)
{
    float t = s1 * 0.1f * 1000.0f;
    t = t + s2 * 0.3f * 1000.0f;
    t = t + s3 * 0.6f * 1000.0f;
    t = t + s4 * 1.0f * 1000.0f;
    return t;
}

/* surface_diagnostics' bulk arm (:337-352).  flags: 1 CQS2 < 1e-3, 2 CHS2 < 1e-3, 4 the SMALL_QV floor acted */
LND_FN void lnd_surface_diagnostics(float hfx, float qfx, float tsk, float qsfc, float chs2, float cqs2, float psfc, float *t2, float *q2, int *flags)
{
    const float rho = psfc / (LND_RD * tsk);
    float q, t;
    int f = 0;
    if (cqs2 < 1.E-3f) { q = qsfc; f |= 1; }
    else q = qsfc - qfx / (rho * cqs2);
    if (chs2 < 1.E-3f) { t = tsk; f |= 2; }
    else t = tsk - hfx / (rho * LND_CP * chs2);
    if (q < LND_SMALL_QV) { q = LND_SMALL_QV; f |= 4; }
    *t2 = t;
    *q2 = q;
    *flags = f;
}

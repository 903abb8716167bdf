// icar_amd/csrc/ra_simple.hip -- the simple radiation scheme (row R1) on gfx950.
//
// Reference algorithm: src/physics/ra_simple.f90 -- ra_simple :191-272, calc_solar_elevation :148-189, cloudfrac :122-146,
// shortwave :84-103, longwave :105-120, ra_simple_init :62-81; relative_humidity (src/utilities/atm_utilities.f90:306-326);
// Time_type%day_of_year / %year_fraction (src/utilities/time_obj.f90:404-480); called by rad(domain, options, dt)
// (src/physics/ra_driver.f90:265-285, which hands it qs = snow + cloud ice + graupel).
//
//   k_ra_simple    lanes along i, one thread per column of the memory row ims:ime, one wave per block.  A tile column first
//                  sums theta * pii and the relative humidity over its lowest five levels (nothing of the column is stored
//                  before), then marches k: the hydrometeor chain ((h + qc) + qs') + qr -- not associative, kept in order -- and,
//                  with runlw, the cooling theta -= (theta pii)**4 coolingrate, four levels' loads (seven streams) in flight;
//                  then the date, the sun, Xu-Randall's cloud fraction, Reiff's shortwave and Idso-Jackson's longwave of the
//                  column.  Columns of ims:ime outside its:ite store the 5e-8 the reference leaves in cloud_cover there
//                  (cloudfrac zeroes its whole result and floors the whole of it, :132-139) and nothing else; swdown / lwdown
//                  outside its:ite are an uninitialised function result in the reference and stay untouched here.
//   k_ra_latitude  cos_lat_m / sin_lat_m of ra_simple_init (:75-76), kept in the context; rerun when the scheme is configured or
//                  ICAR_F_LATITUDE is rewritten.
// REAL(4) throughout in the reference's operation order (no contraction: build.py's -ffp-contract=off; IEEE division and square
// root); sin / cos / asin / exp / x**y are the C library's sinf / cosf / asinf / expf / powf bit for bit (glibc_flt32.h,
// glibc_flt32_trig.h).  How the compiled reference evaluates the two x**4 is taken from its results (tests/golden/ra_simple_*.npz):
// T_air**4 of longwave is ((T T) T) T, the cooling's (theta pii)**4 is (t t)(t t).
// The date: the reference forms `current_date_time - date_to_mjd(year, 1, 1, 0, 0, 0) + offset` in REAL(16); here D = days since
// 1 January 00:00 comes from the model clock and the calendar anchor in FP64 (timestep.hip: icar_rad_run) -- the one part of the
// scheme that is not pinned to the compiled reference.
#include "ctx.h"
#include "glibc_flt32_trig.h"
#include <cstdio>

namespace {
constexpr float pi = 3.1415927f, stefan_boltzmann = 5.67e-8f;         // icar_constants.f90:395-396
constexpr float So = 1367.0f, qcmin = 1e-6f;                          // ra_simple.f90:58-59
constexpr int nrad_layers = 5;                                        // :78

struct RaArgs {
    Dims d;
    int i0, i1, j0, k0, k1;         // 0-based, inclusive
    int calendar, runlw;
    float coolingrate;              // :235
    double D, year_days;            // days since 1 January 00:00 of the model time's year; that year's length
};

// mod(a, 1.0) of REAL(4): exact, with the sign of a (also of a zero result)
__device__ __forceinline__ float mod1(float a) { return __builtin_copysignf(a - __builtin_truncf(a), a); }

__device__ __forceinline__ float relative_humidity(float t, float qv, float p)           // atm_utilities.f90:306-326
{
    const float mr = qv / (1 - qv);
    const float e = mr * p / (0.62197f + mr);
    const float es = 611.2f * gf_expf(17.67f * (t - 273.15f) / (t - 29.65f));
    const float rh = e / es;
    return fminf(1.0f, fmaxf(0.0f, rh));
}

__global__ void __launch_bounds__(64)
k_ra_simple(RaArgs a, float *__restrict__ theta, const float *__restrict__ pii, const float *__restrict__ qv, const float *__restrict__ qc,
            const float *__restrict__ qs, const float *__restrict__ qi, const float *__restrict__ qg, const float *__restrict__ qr,
            const float *__restrict__ p, const float *__restrict__ lon, const float *__restrict__ cos_lat, const float *__restrict__ sin_lat,
            float *__restrict__ swdown, float *__restrict__ lwdown, float *__restrict__ cloud_cover)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = a.j0 + blockIdx.y;
    if (i >= a.d.nx) return;
    const int c2 = i + a.d.nx * j;
    if (i < a.i0 || i > a.i1) { cloud_cover[c2] = 5e-8f; return; }    // :132, :139
    const int sk = a.d.sk;
    int c = a.d.idx(i, a.k0, j);
    // :240-248  T_air and rh over the lowest five levels, from theta before this call cools it
    float T_air = 0.0f, rh = 0.0f;
#pragma unroll
    for (int l = 0; l < nrad_layers; ++l) {
        const float t = theta[c + l * sk] * pii[c + l * sk];
        T_air = T_air + t;
        rh = rh + relative_humidity(t, qv[c + l * sk], p[c + l * sk]);
    }
    T_air = T_air / nrad_layers; rh = rh / nrad_layers;
    if (rh > 1) rh = 1;
    // :250-254 the hydrometeor chain, :264 the cooling
    float h = 0.0f;
    int k = a.k0;
    {   // kts: qc + qs' + qr starts the chain
        const float th = theta[c], pi_ = pii[c];
        h = (qc[c] + ((qs[c] + qi[c]) + qg[c])) + qr[c];
        if (a.runlw) { const float t = th * pi_, t2 = t * t; theta[c] = th - ((t2 * t2) * a.coolingrate); }
        c += sk; ++k;
    }
    for (; k + 3 <= a.k1; k += 4, c += 4 * sk) {
        float th[4], pi_[4], c_[4], s_[4], i_[4], g_[4], r_[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = c + u * sk;
            th[u] = theta[x]; pi_[u] = pii[x]; c_[u] = qc[x]; s_[u] = qs[x]; i_[u] = qi[x]; g_[u] = qg[x]; r_[u] = qr[x];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            h = ((h + c_[u]) + ((s_[u] + i_[u]) + g_[u])) + r_[u];
            if (a.runlw) { const float t = th[u] * pi_[u], t2 = t * t; theta[c + u * sk] = th[u] - ((t2 * t2) * a.coolingrate); }
        }
    }
    for (; k <= a.k1; ++k, c += sk) {
        const float th = theta[c], pi_ = pii[c];
        h = ((h + qc[c]) + ((qs[c] + qi[c]) + qg[c])) + qr[c];
        if (a.runlw) { const float t = th * pi_, t2 = t * t; theta[c] = th - ((t2 * t2) * a.coolingrate); }
    }
    if (h < 0) h = 0;
    // calc_solar_elevation :148-189 with day_of_year / year_fraction (time_obj.f90:404-480)
    const float lo = lon[c2];
    const float off = lo > 180 ? (lo - 360) / 360.0f : lo / 360.0f;
    const double days = a.D + (double)off;
    const float doy = (float)days;
    const float hour_angle = 2 * pi * mod1(doy + 0.5f);
    float day_frac;
    if (a.calendar == 0) day_frac = (float)(days / a.year_days);
    else if (a.calendar == 1) day_frac = doy / 365.0f;
    else day_frac = doy / 360.0f;
    day_frac = mod1(day_frac);
    const float decl = (-0.4091f) * gf_cosf(2.0f * pi / 365.0f * (doy + 10));
    float se = sin_lat[c2] * gf_sinf(decl) + cos_lat[c2] * gf_cosf(decl) * gf_cosf(hour_angle);
    if (se < -1) se = -1; else if (se > 1) se = 1;
    se = gf_asinf(se);
    if (se < 0) se = 0;
    // cloudfrac :122-146
    float temporary = gf_powf((1 - rh) * h, 0.25f);
    if (temporary > 1) temporary = 1;
    if (temporary < 0.0001f) temporary = 0.0001f;
    float cf = h - qcmin;
    if (cf < 5e-8f) cf = 5e-8f;
    cf = gf_powf(rh, 0.25f) * (1 - gf_expf((-2000 * cf) / temporary));
    if (cf < 0) cf = 0;
    if (cf > 1) cf = 1;
    cloud_cover[c2] = cf;
    // shortwave :84-103
    const float s = gf_sinf(se);
    const float sw = So * (1 + 0.035f * gf_cosf(day_frac * 2 * pi)) * s * (0.48f + 0.29f * s);
    swdown[c2] = sw * (1 - (0.75f * gf_powf(cf, 3.4f)));
    if (a.runlw) {                                                    // longwave :105-120
        const float dT = 273.16f - T_air;
        const float emis = 1 - 0.261f * gf_expf((-7.77e-4f) * (dT * dT));
        float lw = emis * stefan_boltzmann * (((T_air * T_air) * T_air) * T_air);
        lw = lw * (1 + 0.2f * cf);
        if (lw > 600.0f) lw = 600.0f;
        lwdown[c2] = lw;
    }
}

__global__ void k_ra_latitude(int n, const float *__restrict__ lat, float *__restrict__ cos_lat, float *__restrict__ sin_lat)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float x = lat[t] / 360.0f * 2 * pi;                         // :75-76
    cos_lat[t] = gf_cosf(x); sin_lat[t] = gf_sinf(x);
}

float *need(icar_hip_ctx *c, int f, const char *member)
{
    if (c->field[f]) return (float *)c->field[f];
    char b[160]; snprintf(b, sizeof b, "ra_simple: domain%%%s (field %d) is not on the device", member, f);
    icar_set_error(b);
    return nullptr;
}
}  // namespace

// ra_simple(theta, pii, qv, qc, qs + qi + qg, qr, p, swdown, lwdown, cloud_cover, lat, lon, date, options, dt, ..., F_runlw) with
// date given as D days since 1 January 00:00 of a year of year_days days
int icar_ra_simple_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte, int runlw,
                       int calendar, double D, double year_days)
{
    if (its < c->ims || ite > c->ime || jts < c->jms || jte > c->jme || kts < c->kms || kte > c->kme) { icar_set_error("ra_simple: tile outside memory bounds"); return 1; }
    if (kts + nrad_layers - 1 > c->kme || kte < kts) { icar_set_error("ra_simple: at least 5 levels (T_air and rh are means over kts .. kts+4, ra_simple.f90:242)"); return 1; }
    if (calendar < 0 || calendar > 2 || !(year_days > 0)) { icar_set_error("ra_simple: calendar is 0 (gregorian), 1 (noleap) or 2 (360-day) with a positive year length"); return 1; }
    if (c->n3 * sizeof(float) >= ((size_t)1 << 31)) { icar_set_error("ra_simple: a field of 2 GiB or more is not supported (32-bit offsets)"); return 1; }
    if (ite < its || jte < jts) return 0;
    if (jte - jts + 1 > 65535) { icar_set_error("ra_simple: more than 65535 rows per call are not supported"); return 1; }
    float *th = need(c, ICAR_F_POTENTIAL_TEMPERATURE, "potential_temperature");
    const float *pii = need(c, ICAR_F_EXNER, "exner"), *qv = need(c, ICAR_F_WATER_VAPOR, "water_vapor"), *qc = need(c, ICAR_F_CLOUD_WATER, "cloud_water_mass");
    const float *qs = need(c, ICAR_F_SNOW, "snow_mass"), *qi = need(c, ICAR_F_CLOUD_ICE, "cloud_ice_mass"), *qg = need(c, ICAR_F_GRAUPEL, "graupel_mass");
    const float *qr = need(c, ICAR_F_RAIN, "rain_mass"), *p = need(c, ICAR_F_PRESSURE, "pressure");
    const float *lat = need(c, ICAR_F_LATITUDE, "latitude"), *lon = need(c, ICAR_F_LONGITUDE, "longitude");
    if (!th || !pii || !qv || !qc || !qs || !qi || !qg || !qr || !p || !lat || !lon) return 1;
    float *sw = icar_field_f(c, ICAR_F_SHORTWAVE, false), *lw = icar_field_f(c, ICAR_F_LONGWAVE, false), *cc = icar_field_f(c, ICAR_F_CLOUD_FRACTION, false);
    if (!sw || !lw || !cc) return 1;
    const int n2 = c->d.nx * c->d.ny;
    if (!c->ra_coslat) { HIPCHK(hipMalloc(&c->ra_coslat, (size_t)2 * n2 * sizeof(float))); c->ra_lat_valid = false; }
    ScopedTimer timer(c, "rad");
    if (!c->ra_lat_valid) {
        hipLaunchKernelGGL(k_ra_latitude, dim3((n2 + 255) / 256), dim3(256), 0, c->stream, n2, lat, c->ra_coslat, c->ra_coslat + n2);
        c->ra_lat_valid = true;
    }
    RaArgs a;
    a.d = c->d; a.i0 = its - c->ims; a.i1 = ite - c->ims; a.j0 = jts - c->jms; a.k0 = kts - c->kms; a.k1 = kte - c->kms;
    a.calendar = calendar; a.runlw = runlw ? 1 : 0;
    a.coolingrate = 1.5f * (dt / 86400.0f) * stefan_boltzmann / 300.0f;
    a.D = D; a.year_days = year_days;
    hipLaunchKernelGGL(k_ra_simple, dim3((c->d.nx + 63) / 64, jte - jts + 1), dim3(64), 0, c->stream, a, th, pii, qv, qc, qs, qi, qg, qr, p, lon,
                       c->ra_coslat, c->ra_coslat + n2, sw, lw, cc);
    HIPCHK(hipGetLastError());
    return 0;
}

// the day of the year of a model time under the calendar anchor of icar_hip_rad_calendar: FP64, rolled once into the next year
int icar_rad_clock(icar_hip_ctx *c, double model_time, double *D, double *year_days)
{
    const IcarStepState &s = c->step;
    if (!s.rad_calendar_set) { icar_set_error("rad: radiation = 2 (kRA_SIMPLE) needs the calendar anchor: call icar_hip_rad_calendar first"); return 1; }
    double d = (model_time - s.rad_year_start) / 86400.0, yd = s.rad_year_days;
    if (d >= yd) { d -= yd; yd = s.rad_next_year_days; }
    *D = d; *year_days = yd;
    return 0;
}

// rad(domain, options, dt) (ra_driver.f90:197-285): the configured scheme on the tile of icar_hip_step_configure
int icar_rad_run(icar_hip_ctx *c, float dt)
{
    if (c->step.radiation != ICAR_RA_SIMPLE) return 0;                 // (kRA_BASIC: the reference's driver has no branch for it)
    const icar_hip_step_config &g = c->step.cfg;
    double D, yd;
    if (icar_rad_clock(c, c->step.model_time, &D, &yd)) return 1;
    return icar_ra_simple_run(c, dt, g.its, g.ite, g.jts, g.jte, g.kts, g.kte, 1, c->step.rad_calendar, D, yd);
}

/* tests/support/ra_oracle.c -- TEST INFRASTRUCTURE: CPU restatement of the simple radiation scheme, src/physics/ra_simple.f90:84-272
 * (ra_simple, calc_solar_elevation, cloudfrac, shortwave, longwave) with relative_humidity (src/utilities/atm_utilities.f90:306-326)
 * and the two Time_type functions it calls (src/utilities/time_obj.f90:404-480), in REAL(4) with the reference's operation order.
 * Compiled with gcc -O2 -ffp-contract=off against the host's libm (sinf, cosf, asinf, expf, powf, fmodf) it is bit-identical to
 * the compiled reference (tests/test_ra_oracle.py holds it to tests/golden/ra_simple_*.npz).
 * Arrays are (ny, nz, nx) C order == Fortran (i, k, j), the 2-D ones (ny, nx); its..kte are 1-based inclusive like the
 * reference's; the memory extent ims:ime is 1:nx.  qs, qi, qg: the driver hands ra_simple `qs + qi + qg` (ra_driver.f90:270-272).
 * The date: D = days since 1 January 00:00 of the model time's year (FP64; the reference holds it in REAL(16)), year_days the
 * length of that year, calendar 0 gregorian, 1 noleap, 2 360-day.
 * Reproduced quirks: cloud_cover(ims:ime, j) outside its:ite becomes 5e-8 on every row jts..jte (cloudfrac zeroes its whole result
 * and floors the whole of it, :132-139); swdown / lwdown outside its:ite are an uninitialised function result in the reference and
 * are left untouched here.  flags (may be NULL, one int per column (ny, nx)): which clip / branch the column took (RA_F_* below). */
#include <math.h>
#include <stdlib.h>
#define IX(i,k,j) ((size_t)(j)*nz*nx + (size_t)(k)*nx + (i))
enum { RA_F_NIGHT = 1, RA_F_ASIN_CLIP = 2, RA_F_LON_GT_180 = 4, RA_F_RH_AT_1 = 8, RA_F_HYDRO_CLIP = 16, RA_F_QC_FLOOR = 32,
       RA_F_TEMP_FLOOR = 64, RA_F_CF_AT_1 = 128, RA_F_LW_CAP = 256, RA_F_CELL = 512 };
static const float pi = 3.1415927f, stefan_boltzmann = 5.67e-8f, So = 1367.0f, qcmin = 1e-6f;   /* icar_constants.f90:395-396, ra_simple.f90:58-59 */

static float relative_humidity(float t, float qv, float p)                /* atm_utilities.f90:306-326 */
{
    float mr = qv / (1 - qv);
    float e = mr * p / (0.62197f + mr);
    float es = 611.2f * expf(17.67f * (t - 273.15f) / (t - 29.65f));
    float rh = e / es;
    return fminf(1.0f, fmaxf(0.0f, rh));
}

static float lon_offset(float lon) { return lon > 180 ? (lon - 360) / 360.0f : lon / 360.0f; }   /* time_obj.f90:414-420 */

int ra_oracle_simple(int nx, int nz, int ny, float *theta, const float *pii, const float *qv, const float *qc, const float *qs,
                     const float *qi, const float *qg, const float *qr, const float *p, float *swdown, float *lwdown, float *cloud_cover,
                     const float *lat, const float *lon, double D, double year_days, int calendar, float dt,
                     int its, int ite, int jts, int jte, int kts, int kte, int runlw, int *flags)
{
    const int nrad_layers = 5;
    if (kts + nrad_layers - 1 > nz) return 1;                              /* the reference reads out of bounds */
    float coolingrate = 1.5f * (dt / 86400.0f) * stefan_boltzmann / 300.0f;      /* :235 */
    float *rh = malloc(sizeof(float) * nx), *T_air = malloc(sizeof(float) * nx), *hyd = malloc(sizeof(float) * nx);
    for (int j = jts - 1; j < jte; j++) {
        for (int i = 0; i < nx; i++) { T_air[i] = 0; rh[i] = 0; }
        for (int k = kts - 1; k < kts - 1 + nrad_layers; k++) for (int i = 0; i < nx; i++) {       /* :242-245 */
            size_t a = IX(i,k,j);
            float t = theta[a] * pii[a];
            T_air[i] = T_air[i] + t;
            rh[i] = rh[i] + relative_humidity(t, qv[a], p[a]);
        }
        for (int i = 0; i < nx; i++) {
            T_air[i] = T_air[i] / nrad_layers; rh[i] = rh[i] / nrad_layers;
            if (rh[i] > 1) rh[i] = 1;
        }
        for (int i = 0; i < nx; i++) { size_t a = IX(i,kts-1,j); hyd[i] = qc[a] + ((qs[a] + qi[a]) + qg[a]) + qr[a]; }   /* :250 */
        for (int k = kts; k < kte; k++) for (int i = 0; i < nx; i++) {                              /* :251-253 */
            size_t a = IX(i,k,j);
            hyd[i] = hyd[i] + qc[a] + ((qs[a] + qi[a]) + qg[a]) + qr[a];
        }
        for (int i = 0; i < nx; i++) {
            size_t c2 = (size_t)j * nx + i;
            int tile = i >= its - 1 && i < ite;
            int fl = tile ? RA_F_CELL : 0;
            float h = hyd[i];
            if (h < 0) { h = 0; fl |= RA_F_HYDRO_CLIP; }                                            /* :254 */
            if (!tile) { cloud_cover[c2] = 5e-8f; if (flags) flags[c2] = 0; continue; }             /* :132, :139 */
            /* calc_solar_elevation :148-189 */
            float off = lon_offset(lon[c2]);
            if (lon[c2] > 180) fl |= RA_F_LON_GT_180;
            float doy = (float)(D + (double)off);                                                   /* time_obj.f90:424 */
            float hour_angle = 2 * pi * fmodf(doy + 0.5f, 1.0f);
            float day_frac;
            if (calendar == 0) day_frac = (float)((D + (double)off) / year_days);                   /* time_obj.f90:461 */
            else if (calendar == 1) day_frac = doy / 365.0f;
            else day_frac = doy / 360.0f;
            day_frac = fmodf(day_frac, 1.0f);
            float decl = (-0.4091f) * cosf(2.0f * pi / 365.0f * (doy + 10));
            float sin_lat = sinf(lat[c2] / 360.0f * 2 * pi), cos_lat = cosf(lat[c2] / 360.0f * 2 * pi);   /* ra_simple_init :75-76 */
            float se = sin_lat * sinf(decl) + cos_lat * cosf(decl) * cosf(hour_angle);
            if (se < -1) { se = -1; fl |= RA_F_ASIN_CLIP; } else if (se > 1) { se = 1; fl |= RA_F_ASIN_CLIP; }
            se = asinf(se);
            if (se < 0) { se = 0; fl |= RA_F_NIGHT; }
            /* cloudfrac :122-146 */
            float r = rh[i];
            if (r >= 1) fl |= RA_F_RH_AT_1;      /* (every term of the mean is <= 1 already: `where(rh > 1)` of :248 cannot fire; the cap shows as rh == 1) */
            float temporary = powf((1 - r) * h, 0.25f);
            if (temporary > 1) temporary = 1;
            if (temporary < 0.0001f) { temporary = 0.0001f; fl |= RA_F_TEMP_FLOOR; }
            float cf = h - qcmin;
            if (cf < 5e-8f) { cf = 5e-8f; fl |= RA_F_QC_FLOOR; }
            cf = powf(r, 0.25f) * (1 - expf((-2000 * cf) / temporary));
            if (cf < 0) cf = 0;
            if (cf > 1) cf = 1;
            if (cf >= 1) fl |= RA_F_CF_AT_1;     /* (a product of two factors <= 1: `where(cloudfrac > 1)` cannot fire either) */
            cloud_cover[c2] = cf;
            /* shortwave :84-103 */
            float s = sinf(se);
            float sw = So * (1 + 0.035f * cosf(day_frac * 2 * pi)) * s * (0.48f + 0.29f * s);
            swdown[c2] = sw * (1 - (0.75f * powf(cf, 3.4f)));
            if (runlw) {                                                                            /* longwave :105-120 */
                float t = T_air[i], d = 273.16f - t;
                float emis = 1 - 0.261f * expf((-7.77e-4f) * (d * d));
                /* T_air**4 as the compiled reference evaluates it HERE: three chained products (the cooling's **4 below is two squarings);
                 * settled by the fixtures, not assumed */
                float lw = emis * stefan_boltzmann * (((t * t) * t) * t);
                lw = lw * (1 + 0.2f * cf);
                if (lw > 600.0f) { lw = 600.0f; fl |= RA_F_LW_CAP; }
                lwdown[c2] = lw;
            }
            if (flags) flags[c2] = fl;
        }
        if (runlw)                                                                                  /* :264 */
            for (int k = kts - 1; k < kte; k++) for (int i = its - 1; i < ite; i++) {
                size_t a = IX(i,k,j);
                float t = theta[a] * pii[a], t2 = t * t;
                theta[a] = theta[a] - ((t2 * t2) * coolingrate);
            }
    }
    free(rh); free(T_air); free(hyd);
    return 0;
}

/* libm's sinf / cosf / asinf on arrays: the host values tests/test_gpu_trig_math.py compares the device's functions with */
void ra_oracle_libm(int which, long n, const float *x, float *y)
{
    for (long t = 0; t < n; t++) y[t] = which == 0 ? sinf(x[t]) : which == 1 ? cosf(x[t]) : asinf(x[t]);
}

// icar_amd/csrc/forcing2d.hip -- the four 2-D variables the reference forces (variables_to_force: sst, shortwave, longwave,
// external_precipitation; src/objects/domain_obj.f90:199, :212, :215, :272) on the device:
//   interpolate_forcing    src/objects/domain_obj.f90:2595-2600 with geo_interp2d, src/utilities/geo_reader.f90:1142-1182
//   update_delta_fields    src/objects/domain_obj.f90:2355-2356
//   apply_forcing          src/objects/domain_obj.f90:2400-2402 and the precipitation sum :2438-2445
// The per-cell arithmetic is forcing2d_cell.h (shared with the CPU restatement).  Lanes run along i.  The look-up tables are the mass
// grid's geolut of icar_hip_forcing_configure (forcing.hip validated every index before it stored them: the kernel gathers through
// them unchecked).  data_2d of sst / shortwave / longwave is the field slot; external_precipitation has no slot and lives here.
#include "ctx.h"
#include <cstring>
#include <cstdio>
#include <cmath>

#define F2_FN __device__ __forceinline__
#include "forcing2d_cell.h"

struct Forcing2dState {
    float *lo[ICAR_FORCED2D_N] = {nullptr};            // input_data%data_2d (nx_f, ny_f), as uploaded
    int lo_nx[ICAR_FORCED2D_N] = {0}, lo_ny[ICAR_FORCED2D_N] = {0};
    float *dqdt[ICAR_FORCED2D_N] = {nullptr};          // dqdt_2d (nx, ny)
    float *ext = nullptr;                              // external_precipitation%data_2d (nx, ny)
    int enabled[ICAR_FORCED2D_N] = {0}, n_enabled = 0; // icar_hip_forcing2d_enable's list, in its order
};

static const int kSlot[ICAR_FORCED2D_N] = {ICAR_F_SST, ICAR_F_SHORTWAVE, ICAR_F_LONGWAVE, -1};

struct F2Interp { const float *lo[ICAR_FORCED2D_N]; float *out[ICAR_FORCED2D_N]; };
struct F2Delta { float *dqdt[ICAR_FORCED2D_N]; const float *data[ICAR_FORCED2D_N]; };
struct F2Apply { float *x[ICAR_FORCED2D_N]; const float *dq[ICAR_FORCED2D_N]; int n; const float *ext; double *acc; };

// geo_interp2d over the whole memory ims:ime, jms:jme: a thread owns one cell of one variable (blockIdx.z).  The cell's four x, four y
// and its weights are one 16-byte load each (the tables are (4, nx, ny): a cell's tuple is aligned), coalesced along i; the four
// gathers go to the small forcing array, which stays in cache.
__global__ void __launch_bounds__(64) k_geo_interp2d(IcarGeo2d g, F2Interp v)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y, m = blockIdx.z;
    if (i >= g.nx) return;
    const int c = i + g.nx * j;                                  // every grid has fewer than 2^31 cells (forcing_configure)
    const int4 x = g.x[c], y = g.y[c]; const float4 w = g.w[c];
    const int x4[4] = {x.x, x.y, x.z, x.w}, y4[4] = {y.x, y.y, y.z, y.w};
    const float w4[3] = {w.x, w.y, w.z};
    v.out[m][c] = f2_geo_cell(v.lo[m], g.nx_f, x4, y4, w4);
}

__global__ void __launch_bounds__(256) k_delta2d(F2Delta a, unsigned n, double dt)
{
    const unsigned m = blockIdx.y;
    float *__restrict__ dq = a.dqdt[m]; const float *__restrict__ x = a.data[m];
    for (unsigned t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) dq[t] = f2_delta(dq[t], x[t], dt);
}

// apply_forcing's 2-D part of one sub-step: every enabled variable (external_precipitation among them, :2402) and then, from the
// precipitation rate just updated, the sum :2443 -- the order of the reference's statements, cell by cell
__global__ void __launch_bounds__(256) k_apply2d(F2Apply a, unsigned n, double dt)
{
    for (unsigned t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        for (int m = 0; m < ICAR_FORCED2D_N; ++m)
            if (m < a.n) a.x[m][t] = f2_apply(a.x[m][t], a.dq[m][t], dt);
        if (a.acc) a.acc[t] = f2_precip(a.acc[t], a.ext[t], dt);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
void icar_forcing2d_free(icar_hip_ctx *c)
{
    Forcing2dState *s = c->forcing2d;
    if (!s) return;
    for (int m = 0; m < ICAR_FORCED2D_N; ++m) { if (s->lo[m]) hipFree(s->lo[m]); if (s->dqdt[m]) hipFree(s->dqdt[m]); }
    if (s->ext) hipFree(s->ext);
    delete s;
    c->forcing2d = nullptr;
}

static int refuse(const char *who, const char *fmt, long a = 0, long b = 0, long d = 0, long e = 0)
{
    char m[256], t[200];
    snprintf(t, sizeof t, fmt, a, b, d, e);
    snprintf(m, sizeof m, "%s: %s", who, t);
    icar_set_error(m);
    return 1;
}

static Forcing2dState *state(icar_hip_ctx *c)
{
    if (!c->forcing2d) c->forcing2d = new Forcing2dState();
    return c->forcing2d;
}

static size_t n2(const icar_hip_ctx *c) { return (size_t)c->d.nx * c->d.ny; }

// data_2d of a variable as it is on the device now (null: not there)
static float *data_of(icar_hip_ctx *c, int v)
{
    if (kSlot[v] >= 0) return (float *)c->field[kSlot[v]];
    return c->forcing2d ? c->forcing2d->ext : nullptr;
}

static int zeros(icar_hip_ctx *c, float **p)
{
    if (*p) return 0;
    HIPCHK(hipMalloc(p, n2(c) * sizeof(float)));
    HIPCHK(hipMemsetAsync(*p, 0, n2(c) * sizeof(float), c->stream));
    return 0;
}

// data_2d or dqdt_2d of a variable, created (zeros) if needed
static float *make(icar_hip_ctx *c, int v, int dqdt)
{
    Forcing2dState *s = state(c);
    if (dqdt) return zeros(c, &s->dqdt[v]) ? nullptr : s->dqdt[v];
    if (kSlot[v] >= 0) return icar_field_f(c, kSlot[v], false);
    return zeros(c, &s->ext) ? nullptr : s->ext;
}

// a list of variables: ids in range, none twice
static int list_check(const char *who, const int *which, int n)
{
    if (n < 0 || n > ICAR_FORCED2D_N) return refuse(who, "bad variable count %ld", n);
    for (int m = 0; m < n; ++m) {
        if (which[m] < 0 || which[m] >= ICAR_FORCED2D_N) return refuse(who, "bad forced 2-D variable id %ld", which[m]);
        for (int q = 0; q < m; ++q) if (which[q] == which[m]) return refuse(who, "forced 2-D variable %ld is listed twice", which[m]);
    }
    return 0;
}

static int configured(icar_hip_ctx *c, const char *who, IcarGeo2d *g)
{
    if (!icar_forcing_mass_geo(c, g)) return refuse(who, "icar_hip_forcing_configure has not been called");
    return 0;
}

// everything the interpolation refuses, before anything is allocated or launched
static int interpolate_check(icar_hip_ctx *c, const char *who, const int *which, int n, IcarGeo2d *g)
{
    if (configured(c, who, g) || list_check(who, which, n)) return 1;
    const Forcing2dState *s = c->forcing2d;
    for (int m = 0; m < n; ++m) {
        const int v = which[m];
        if (!s || !s->lo[v]) return refuse(who, "forced 2-D variable %ld has no forcing data: icar_hip_forcing2d_upload comes first", v);
        if (s->lo_nx[v] != g->nx_f || s->lo_ny[v] != g->ny_f)
            return refuse(who, "the forcing data of a 2-D variable are %ld x %ld, the mass grid's look-up tables were made for %ld x %ld", s->lo_nx[v], s->lo_ny[v], g->nx_f, g->ny_f);
    }
    return 0;
}

static int interpolate_run(icar_hip_ctx *c, const IcarGeo2d &g, const int *which, int n, int update)
{
    if (n == 0) return 0;
    Forcing2dState *s = state(c);
    F2Interp a;
    for (int m = 0; m < n; ++m) {                               // every destination exists before the launch
        a.lo[m] = s->lo[which[m]];
        if (!(a.out[m] = make(c, which[m], update))) return 1;
    }
    ScopedTimer t(c, "forcing2d_interp");
    k_geo_interp2d<<<dim3((g.nx + 63) / 64, g.ny, n), 64, 0, c->stream>>>(g, a);
    HIPCHK(hipGetLastError());
    return 0;
}

static int delta_check(icar_hip_ctx *c, const char *who, const int *which, int n, double dt, bool dqdt_will_exist)
{
    if (list_check(who, which, n)) return 1;
    if (!(dt > 0.0) || !std::isfinite(dt)) return refuse(who, "dt must be a positive number of seconds");
    const Forcing2dState *s = c->forcing2d;
    for (int m = 0; m < n; ++m) {
        if (!dqdt_will_exist && (!s || !s->dqdt[which[m]])) return refuse(who, "forced 2-D variable %ld has no dqdt_2d on the device", which[m]);
        if (!data_of(c, which[m])) return refuse(who, "forced 2-D variable %ld has no data_2d on the device", which[m]);
    }
    return 0;
}

static unsigned blocks_of(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 2048); }

static int delta_run(icar_hip_ctx *c, const int *which, int n, double dt)
{
    if (n == 0) return 0;
    Forcing2dState *s = state(c);
    F2Delta a;
    for (int m = 0; m < n; ++m) {
        a.dqdt[m] = s->dqdt[which[m]];
        a.data[m] = data_of(c, which[m]);
    }
    ScopedTimer t(c, "forcing2d_delta");
    k_delta2d<<<dim3(blocks_of(n2(c)), n), 256, 0, c->stream>>>(a, (unsigned)n2(c), dt);
    HIPCHK(hipGetLastError());
    return 0;
}

// apply_forcing's 2-D statements for the enabled set: one launch.  A variable whose data_2d or dqdt_2d is not on the device is not
// `associated` and is passed over; so is the sum while there is no accumulated precipitation (:2442) or no external_precipitation
int icar_forcing2d_apply_run(icar_hip_ctx *c, double dt)
{
    Forcing2dState *s = c->forcing2d;
    if (!s || !s->n_enabled) return 0;
    F2Apply a; a.n = 0; a.ext = nullptr; a.acc = nullptr;
    for (int m = 0; m < ICAR_FORCED2D_N; ++m) { a.x[m] = nullptr; a.dq[m] = nullptr; }
    for (int m = 0; m < s->n_enabled; ++m) {
        const int v = s->enabled[m];
        float *x = data_of(c, v);
        if (v == ICAR_FORCED2D_EXTERNAL_PRECIPITATION && x && c->field[ICAR_F_PRECIPITATION]) { a.ext = x; a.acc = (double *)c->field[ICAR_F_PRECIPITATION]; }
        if (!x || !s->dqdt[v]) continue;
        a.x[a.n] = x; a.dq[a.n] = s->dqdt[v]; ++a.n;
    }
    if (!a.n && !a.acc) return 0;
    ScopedTimer t(c, "forcing2d_apply");
    k_apply2d<<<blocks_of(n2(c)), 256, 0, c->stream>>>(a, (unsigned)n2(c), dt);
    HIPCHK(hipGetLastError());
    return 0;
}

// icar_hip_forcing_step's share (forcing.hip): what the enabled set would be refused for, before the first launch of the step ...
int icar_forcing2d_step_check(icar_hip_ctx *c, const char *who, double dt)
{
    const Forcing2dState *s = c->forcing2d;
    if (!s || !s->n_enabled) return 0;
    IcarGeo2d g;
    return interpolate_check(c, who, s->enabled, s->n_enabled, &g) || delta_check(c, who, s->enabled, s->n_enabled, dt, true);
}

// ... and the interpolation (update) and the delta themselves
int icar_forcing2d_step_run(icar_hip_ctx *c, double dt)
{
    Forcing2dState *s = c->forcing2d;
    if (!s || !s->n_enabled) return 0;
    IcarGeo2d g;
    if (!icar_forcing_mass_geo(c, &g)) return refuse("forcing_step", "icar_hip_forcing_configure has not been called");
    return interpolate_run(c, g, s->enabled, s->n_enabled, 1) || delta_run(c, s->enabled, s->n_enabled, dt);
}

extern "C" {

int icar_hip_forcing2d_upload(icar_hip_ctx *c, int which, const float *lo, int nx_f, int ny_f)
{
    const char *who = "forcing2d_upload";
    if (icar_enter(c, who, lo != nullptr)) return 1;
    IcarGeo2d g;
    if (configured(c, who, &g)) return 1;
    if (which < 0 || which >= ICAR_FORCED2D_N) return refuse(who, "bad forced 2-D variable id %ld", which);
    if (nx_f != g.nx_f || ny_f != g.ny_f) return refuse(who, "the forcing data are %ld x %ld, the mass grid's look-up tables were made for %ld x %ld", nx_f, ny_f, g.nx_f, g.ny_f);
    Forcing2dState *s = state(c);
    const size_t n = (size_t)nx_f * ny_f;
    if (s->lo[which] && (size_t)s->lo_nx[which] * s->lo_ny[which] != n) { hipFree(s->lo[which]); s->lo[which] = nullptr; }
    if (!s->lo[which]) HIPCHK(hipMalloc(&s->lo[which], n * sizeof(float)));
    s->lo_nx[which] = nx_f; s->lo_ny[which] = ny_f;
    HIPCHK(hipMemcpyAsync(s->lo[which], lo, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_forcing2d_download(icar_hip_ctx *c, int which, float *lo, size_t count)
{
    const char *who = "forcing2d_download";
    if (icar_enter(c, who, lo != nullptr)) return 1;
    const Forcing2dState *s = c->forcing2d;
    if (which < 0 || which >= ICAR_FORCED2D_N) return refuse(who, "bad forced 2-D variable id %ld", which);
    if (!s || !s->lo[which]) return refuse(who, "forced 2-D variable %ld has no forcing data", which);
    if (count != (size_t)s->lo_nx[which] * s->lo_ny[which]) return refuse(who, "count does not match the %ld elements uploaded", (long)s->lo_nx[which] * s->lo_ny[which]);
    HIPCHK(hipMemcpyAsync(lo, s->lo[which], count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_interpolate_forcing_2d(icar_hip_ctx *c, const int *which, int n, int update)
{
    const char *who = "interpolate_forcing_2d";
    if (icar_enter(c, who, n <= 0 || which)) return 1;
    IcarGeo2d g;
    if (interpolate_check(c, who, which, n, &g)) return 1;
    return interpolate_run(c, g, which, n, update);
}

int icar_hip_update_delta_fields_2d(icar_hip_ctx *c, const int *which, int n, double dt_seconds)
{
    const char *who = "update_delta_fields_2d";
    if (icar_enter(c, who, n <= 0 || which)) return 1;
    IcarGeo2d g;
    if (configured(c, who, &g) || delta_check(c, who, which, n, dt_seconds, false)) return 1;
    return delta_run(c, which, n, dt_seconds);
}

int icar_hip_apply_forcing_2d(icar_hip_ctx *c, double dt_seconds)
{
    const char *who = "apply_forcing_2d";
    if (icar_enter(c, who)) return 1;
    IcarGeo2d g;
    if (configured(c, who, &g)) return 1;
    if (!(dt_seconds > 0.0) || !std::isfinite(dt_seconds)) return refuse(who, "dt must be a positive number of seconds");
    return icar_forcing2d_apply_run(c, dt_seconds);
}

int icar_hip_forcing2d_enable(icar_hip_ctx *c, const int *which, int n)
{
    const char *who = "forcing2d_enable";
    if (icar_enter(c, who, n <= 0 || which)) return 1;
    IcarGeo2d g;
    if (configured(c, who, &g) || list_check(who, which, n)) return 1;
    Forcing2dState *s = state(c);
    s->n_enabled = n;
    for (int m = 0; m < n; ++m) s->enabled[m] = which[m];
    return 0;
}

static int getset(icar_hip_ctx *c, const char *who, int which, int what, float *host, bool to_device)
{
    if (icar_enter(c, who, host != nullptr)) return 1;
    if (which < 0 || which >= ICAR_FORCED2D_N) return refuse(who, "bad forced 2-D variable id %ld", which);
    if (what != ICAR_FORCED2D_DATA && what != ICAR_FORCED2D_DQDT) return refuse(who, "what = %ld is neither ICAR_FORCED2D_DATA nor ICAR_FORCED2D_DQDT", what);
    float *p = what == ICAR_FORCED2D_DQDT ? (c->forcing2d ? c->forcing2d->dqdt[which] : nullptr) : data_of(c, which);
    if (!to_device && !p) return refuse(who, what == ICAR_FORCED2D_DQDT ? "forced 2-D variable %ld has no dqdt_2d on the device" : "forced 2-D variable %ld has no data_2d on the device", which);
    if (to_device && !(p = make(c, which, what == ICAR_FORCED2D_DQDT))) return 1;
    if (to_device) HIPCHK(hipMemcpyAsync(p, host, n2(c) * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, p, n2(c) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_forcing2d_get(icar_hip_ctx *c, int which, int what, float *host) { return getset(c, "forcing2d_get", which, what, host, false); }
int icar_hip_forcing2d_set(icar_hip_ctx *c, int which, int what, const float *host) { return getset(c, "forcing2d_set", which, what, (float *)host, true); }

}  // extern "C"

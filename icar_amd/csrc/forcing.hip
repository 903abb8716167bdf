// icar_amd/csrc/forcing.hip -- the forcing update of the reference's outer loop (src/main/driver.f90:133-137) on the device:
//   domain%interpolate_forcing(forcing, update)   src/objects/domain_obj.f90:2559-2643 with interpolate_variable :2709-2809 and
//                                                 adjust_pressure :2656-2702
//   domain%update_delta_fields(dt)                src/objects/domain_obj.f90:2339-2372
// The per-cell arithmetic is forcing_interp.h (shared with the CPU restatement); the smoothing of u / v is linear_winds.hip's
// smooth_array_3d pair (k_lw_rowmeans, k_lw_colsmooth).  Lanes run along i.  The look-up tables (geo_LUT, vLUT) are made by the host
// at init time and validated here, index by index, before anything is stored: the kernels gather through them unchecked.
#include "ctx.h"
#include "glibc_flt32.h"
#include <vector>
#include <cstring>
#include <cstdio>
#include <cmath>

#define FI_FN __device__ __forceinline__
#define FI_EXPF gf_expf
#define FI_POWF gf_powf
#include "forcing_interp.h"

#define FORCING_MAXV 12             // variables of one k_forcing_mass launch

struct FGeoDev {                    // one grid's tables on the device
    int4 *x = nullptr, *y = nullptr; float4 *w = nullptr;      // geolut (4, nx, ny)
    int2 *vz = nullptr; float2 *vw = nullptr;                  // vert_lut (2, nx, nz, ny)
    int nx = 0, ny = 0, nx_f = 0, nz_f = 0, ny_f = 0, i0 = 0, j0 = 0;
    bool set = false;
};
struct ForcingState {
    bool configured = false;
    FGeoDev mass, u, v;
    int nsmooth = 0;
    float *z_f = nullptr, *z_d = nullptr;                      // forcing%geo%z (nx, nz_f, ny), domain%geo%z (nx, nz, ny)
    float *lo[ICAR_N_FIELD_SLOTS] = {nullptr};                 // the forcing's own arrays (input_data%data_3d), as uploaded
    int lo_dims[ICAR_N_FIELD_SLOTS][3] = {{0}};
    float *p_nv = nullptr, *th_nv = nullptr;                   // pressure and potential temperature without vertical interpolation (n3)
    float *ext = nullptr; double *rowmeans = nullptr;          // temp_3d on the extended grid, smooth_array's row means
    size_t ext_n = 0, rowmeans_n = 0;
};

struct FVars { const float *lo[FORCING_MAXV]; float *out[FORCING_MAXV]; int n; };
struct FGeoArg { const int4 *x, *y; const float4 *w; const int2 *vz; const float2 *vw; int nx, ny, nx_f, nz_f; };

// geo_interp + vinterp fused: a thread owns one output column position (i, j) and walks k.  The column's corners and weights are
// loaded once; for every level the two horizontal interpolations vert_lut names are evaluated from the (cache-resident) forcing
// array and rounded to REAL(4) where the reference stores temp_3d; every variable of the launch shares the vert_lut entry.
__global__ void __launch_bounds__(64) k_forcing_mass(FGeoArg g, int nz, FVars v)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= g.nx) return;
    const int c = i + g.nx * j;                                  // every grid has fewer than 2^31 cells (forcing_configure)
    const int4 x = g.x[c], y = g.y[c]; const float4 w = g.w[c];
    const int c4[4] = {fi_corner(x.x, y.x, g.nx_f, g.nz_f), fi_corner(x.y, y.y, g.nx_f, g.nz_f), fi_corner(x.z, y.z, g.nx_f, g.nz_f),
                       fi_corner(x.w, y.w, g.nx_f, g.nz_f)};
    const float w4[3] = {w.x, w.y, w.z};
    for (int k = 0; k < nz; ++k) {
        const int o = i + g.nx * (k + nz * j);
        const int2 z = g.vz[o]; const float2 zw = g.vw[o];
        for (int m = 0; m < v.n; ++m) {
            const float a = fi_geo_cell(v.lo[m], g.nx_f, g.nz_f, c4, w4, z.x);
            const float b = fi_geo_cell(v.lo[m], g.nx_f, g.nz_f, c4, w4, z.y);
            v.out[m][o] = fi_vinterp(a, zw.x, b, zw.y);
        }
    }
}

// geo_interp and the vert_interp = .false. branch of interpolate_variable: output level k is level min(k, nz_f) of temp_3d
__global__ void __launch_bounds__(64) k_forcing_mass_novert(FGeoArg g, int nz, FVars v)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= g.nx) return;
    const int c = i + g.nx * j;                                  // every grid has fewer than 2^31 cells (forcing_configure)
    const int4 x = g.x[c], y = g.y[c]; const float4 w = g.w[c];
    const int c4[4] = {fi_corner(x.x, y.x, g.nx_f, g.nz_f), fi_corner(x.y, y.y, g.nx_f, g.nz_f), fi_corner(x.z, y.z, g.nx_f, g.nz_f),
                       fi_corner(x.w, y.w, g.nx_f, g.nz_f)};
    const float w4[3] = {w.x, w.y, w.z};
    for (int k = 0; k < nz; ++k) {
        const int o = i + g.nx * (k + nz * j);
        for (int m = 0; m < v.n; ++m) v.out[m][o] = fi_geo_cell(v.lo[m], g.nx_f, g.nz_f, c4, w4, k + 1);
    }
}

// adjust_pressure: one thread per column, the findz march and the exponential
__global__ void __launch_bounds__(64) k_adjust_pressure(int nx, int nz, int nz_f, int ny, const float *__restrict__ p_in, const float *__restrict__ th_in,
                                                        const float *__restrict__ z_in, const float *__restrict__ z_out, float *__restrict__ p_out)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= nx) return;
    const size_t col = (size_t)i + (size_t)nx * nz * j;
    fi_adjust_pressure_column(p_in + col, th_in + col, z_in + (size_t)i + (size_t)nx * nz_f * j, z_out + col, p_out + col, nz, (size_t)nx, nullptr);
}

// var_data = temp_3d(i0+1 : i0+nxd, :, j0+1 : j0+nyd) (:2783-2785, :2804-2806)
__global__ void k_forcing_box(const float *__restrict__ ext, int nxe, int nz, int i0, int j0, float *__restrict__ out, int nxd, int nyd)
{
    const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y, j = blockIdx.z;
    if (i >= nxd) return;
    out[(size_t)i + (size_t)nxd * ((size_t)k + (size_t)nz * j)] = ext[(size_t)(i + i0) + (size_t)nxe * ((size_t)k + (size_t)nz * (j + j0))];
}

struct FDelta { float *dqdt[ICAR_N_FIELD_SLOTS]; const float *data[ICAR_N_FIELD_SLOTS]; unsigned n[ICAR_N_FIELD_SLOTS]; };
__global__ void k_update_delta(FDelta a, double dt)
{
    const unsigned f = blockIdx.y;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < a.n[f]; t += gridDim.x * blockDim.x) a.dqdt[f][t] = fi_delta(a.dqdt[f][t], a.data[f][t], dt);
}

// ------------------------------------------------------------------------------------------------------------------------------------
static void geo_free(FGeoDev &g)
{
    void *p[] = {g.x, g.y, g.w, g.vz, g.vw};
    for (void *q : p) if (q) hipFree(q);
    g = FGeoDev();
}

void icar_forcing_free(icar_hip_ctx *c)
{
    ForcingState *s = c->forcing;
    if (!s) return;
    geo_free(s->mass); geo_free(s->u); geo_free(s->v);
    for (float *p : s->lo) if (p) hipFree(p);
    void *q[] = {s->z_f, s->z_d, s->p_nv, s->th_nv, s->ext, s->rowmeans};
    for (void *p : q) if (p) hipFree(p);
    delete s;
    c->forcing = nullptr;
}

static int refuse(const char *who, const char *fmt, long a = 0, long b = 0, long d = 0, long e = 0)
{
    char m[256], t[200];
    snprintf(t, sizeof t, fmt, a, b, d, e);
    snprintf(m, sizeof m, "%s: %s", who, t);
    icar_set_error(m);
    return 1;
}

// every index of a grid's tables, on the host, before anything is stored
static int geo_validate(const char *name, const icar_hip_forcing_geo *g, int nz)
{
    char who[64]; snprintf(who, sizeof who, "forcing_configure (%s)", name);
    if (!g->x || !g->y || !g->w || !g->z || !g->zw) return refuse(who, "a null table");
    if (g->nx < 1 || g->ny < 1 || g->nx_f < 1 || g->nz_f < 1 || g->ny_f < 1) return refuse(who, "an extent below 1");
    if ((size_t)g->nx * nz * g->ny >= ((size_t)1 << 31) || (size_t)g->nx_f * g->nz_f * g->ny_f >= ((size_t)1 << 31)) return refuse(who, "grid too large for 32-bit indexing");
    const size_t n2 = (size_t)g->nx * g->ny;
    for (size_t t = 0; t < 4 * n2; ++t) {
        if (g->x[t] < 1 || g->x[t] > g->nx_f) return refuse(who, "geolut%%x(%ld) = %ld is outside 1..%ld", (long)t + 1, g->x[t], g->nx_f);
        if (g->y[t] < 1 || g->y[t] > g->ny_f) return refuse(who, "geolut%%y(%ld) = %ld is outside 1..%ld", (long)t + 1, g->y[t], g->ny_f);
    }
    for (size_t t = 0; t < 2 * n2 * nz; ++t)
        if (g->z[t] < 1 || g->z[t] > g->nz_f) return refuse(who, "vert_lut%%z(%ld) = %ld is outside 1..%ld", (long)t + 1, g->z[t], g->nz_f);
    return 0;
}

static int geo_store(icar_hip_ctx *c, FGeoDev &d, const icar_hip_forcing_geo *g, int nz)
{
    geo_free(d);
    const size_t n2 = (size_t)g->nx * g->ny, n3 = n2 * nz;
    HIPCHK(hipMalloc(&d.x, n2 * sizeof(int4))); HIPCHK(hipMalloc(&d.y, n2 * sizeof(int4))); HIPCHK(hipMalloc(&d.w, n2 * sizeof(float4)));
    HIPCHK(hipMalloc(&d.vz, n3 * sizeof(int2))); HIPCHK(hipMalloc(&d.vw, n3 * sizeof(float2)));
    HIPCHK(hipMemcpyAsync(d.x, g->x, n2 * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d.y, g->y, n2 * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d.w, g->w, n2 * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d.vz, g->z, n3 * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d.vw, g->zw, n3 * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    d.nx = g->nx; d.ny = g->ny; d.nx_f = g->nx_f; d.nz_f = g->nz_f; d.ny_f = g->ny_f; d.i0 = g->i0; d.j0 = g->j0;
    d.set = true;
    return 0;
}

bool icar_forcing_mass_geo(const icar_hip_ctx *c, IcarGeo2d *g)
{
    const ForcingState *s = c->forcing;
    if (!s || !s->configured || !s->mass.set) return false;
    *g = IcarGeo2d{s->mass.x, s->mass.y, s->mass.w, s->mass.nx, s->mass.ny, s->mass.nx_f, s->mass.ny_f};
    return true;
}

static FGeoArg geo_arg(const FGeoDev &d) { return FGeoArg{d.x, d.y, d.w, d.vz, d.vw, d.nx, d.ny, d.nx_f, d.nz_f}; }

static int forcing_configure_run(icar_hip_ctx *c, const icar_hip_forcing_geo *mass, const icar_hip_forcing_geo *u, const icar_hip_forcing_geo *v,
                                 int nsmooth, const float *forcing_z, const float *domain_z, int time_varying_z)
{
    const char *who = "forcing_configure";
    const Dims d = c->d;
    if (time_varying_z) return refuse(who, "time_varying_z is not built (vLUT_forcing, vinterp axis 3)");
    if (!mass) return refuse(who, "the mass grid's tables are required");
    if (mass->nx != d.nx || mass->ny != d.ny) return refuse(who, "the mass grid's tables are %ld x %ld, the context's tile is %ld x %ld", mass->nx, mass->ny, d.nx, d.ny);
    if (geo_validate("mass", mass, d.nz)) return 1;
    if ((forcing_z == nullptr) != (domain_z == nullptr)) return refuse(who, "forcing%%geo%%z and domain%%geo%%z come together");
    if (forcing_z && mass->nz_f < d.nz)
        return refuse(who, "adjust_pressure indexes forcing%%geo%%z with the model's %ld levels, the forcing has %ld (the reference reads out of bounds)", d.nz, mass->nz_f);
    if ((u == nullptr) != (v == nullptr)) return refuse(who, "the u and v grids' tables come together");
    if (u) {
        if (nsmooth < 1) return refuse(who, "nsmooth = %ld: smooth_array needs a window of at least 1", nsmooth);
        const icar_hip_forcing_geo *gs[2] = {u, v};
        for (int m = 0; m < 2; ++m) {
            const icar_hip_forcing_geo *g = gs[m];
            const char *nm = m ? "v" : "u";
            if (geo_validate(nm, g, d.nz)) return 1;
            const int nxd = d.nx + (m == 0), nyd = d.ny + (m == 1);
            if (g->i0 < 0 || g->j0 < 0 || g->i0 + nxd > g->nx || g->j0 + nyd > g->ny) {
                char t[64]; snprintf(t, sizeof t, "forcing_configure (%s)", nm);
                return refuse(t, "the tile (offset %ld, %ld) does not lie inside the extended grid %ld x %ld", g->i0, g->j0, g->nx, g->ny);
            }
            if (nsmooth > g->nx) {
                char t[64]; snprintf(t, sizeof t, "forcing_configure (%s)", nm);
                return refuse(t, "nsmooth = %ld is wider than the extended grid's %ld columns (smooth_array reads rowmeans(2:windowsize))", nsmooth, g->nx);
            }
        }
    }
    // nothing has been stored so far
    if (!c->forcing) c->forcing = new ForcingState();
    ForcingState *s = c->forcing;
    s->configured = false;
    if (geo_store(c, s->mass, mass, d.nz)) return 1;
    if (u) { if (geo_store(c, s->u, u, d.nz) || geo_store(c, s->v, v, d.nz)) return 1; }
    else { geo_free(s->u); geo_free(s->v); }
    s->nsmooth = nsmooth;
    if (s->z_f) { hipFree(s->z_f); s->z_f = nullptr; }
    if (s->z_d) { hipFree(s->z_d); s->z_d = nullptr; }
    if (forcing_z) {
        const size_t nf = (size_t)d.nx * mass->nz_f * d.ny;
        HIPCHK(hipMalloc(&s->z_f, nf * sizeof(float))); HIPCHK(hipMalloc(&s->z_d, c->n3 * sizeof(float)));
        HIPCHK(hipMemcpyAsync(s->z_f, forcing_z, nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->z_d, domain_z, c->n3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    s->configured = true;
    return 0;
}

static int forcing_upload_run(icar_hip_ctx *c, int f, const float *lo, int nx_f, int nz_f, int ny_f)
{
    const char *who = "forcing_upload";
    if (f < 0 || f >= ICAR_N_FIELD_SLOTS) return refuse(who, "bad field id %ld", f);
    if (!icar_field_is_3d(c, f)) return refuse(who, "field %ld is 2-D: only 3-D forced fields are built (geo_interp2d is not)", f);
    if (nx_f < 1 || nz_f < 1 || ny_f < 1 || (size_t)nx_f * nz_f * ny_f >= ((size_t)1 << 31)) return refuse(who, "bad extents");
    if (!c->forcing) c->forcing = new ForcingState();
    ForcingState *s = c->forcing;
    const size_t n = (size_t)nx_f * nz_f * ny_f;
    int *dm = s->lo_dims[f];
    if (s->lo[f] && (size_t)dm[0] * dm[1] * dm[2] != n) { hipFree(s->lo[f]); s->lo[f] = nullptr; }
    if (!s->lo[f]) HIPCHK(hipMalloc(&s->lo[f], n * sizeof(float)));
    dm[0] = nx_f; dm[1] = nz_f; dm[2] = ny_f;
    HIPCHK(hipMemcpyAsync(s->lo[f], lo, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static int ensure(void **p, size_t &have, size_t want, size_t elem)
{
    if (*p && have >= want) return 0;
    if (*p) hipFree(*p);
    *p = nullptr; have = 0;
    HIPCHK(hipMalloc(p, want * elem));
    have = want;
    return 0;
}

// smooth_array(a, windowsize = w, ydim = 3) in place on a (nx, nz, ny)
static int smooth_run(icar_hip_ctx *c, ForcingState *s, float *a, int nx, int nz, int ny, int w)
{
    Dims d; d.nx = nx; d.nz = nz; d.ny = ny; d.sk = nx; d.sj = nx * nz;
    if (ensure((void **)&s->rowmeans, s->rowmeans_n, (size_t)nx * nz * ny, sizeof(double))) return 1;
    k_lw_rowmeans<<<dim3((nx + 63) / 64, nz), 64, 0, c->stream>>>(d, w, a, s->rowmeans);
    k_lw_colsmooth<<<dim3((nz + 63) / 64, ny), 64, 0, c->stream>>>(d, w, s->rowmeans, a);
    return 0;
}

static float *destination(icar_hip_ctx *c, int f, int update)
{
    if (!update) return icar_field_f(c, f, false);
    if (!c->dqdt[f]) {
        const size_t bytes = icar_field_count(c, f) * sizeof(float);
        if (icar_hip_check(hipMalloc(&c->dqdt[f], bytes), "hipMalloc(dqdt)")) return nullptr;
        if (icar_hip_check(hipMemsetAsync(c->dqdt[f], 0, bytes, c->stream), "hipMemset(dqdt)")) return nullptr;
    }
    return c->dqdt[f];
}

// everything interpolate_forcing refuses, before anything is allocated or launched
static int interpolate_forcing_check(icar_hip_ctx *c, const char *who, const int *fields, int n, int pressure_field, int theta_field)
{
    ForcingState *s = c->forcing;
    if (!s || !s->configured) return refuse(who, "icar_hip_forcing_configure has not been called");
    if (n < 0 || n > ICAR_N_FIELD_SLOTS) return refuse(who, "bad field count %ld", n);
    bool has_p = false;
    for (int m = 0; m < n; ++m) {
        const int f = fields[m];
        if (f < 0 || f >= ICAR_N_FIELD_SLOTS) return refuse(who, "bad field id %ld", f);
        if (!icar_field_is_3d(c, f)) return refuse(who, "field %ld is 2-D: only 3-D forced fields are built (geo_interp2d is not)", f);
        for (int q = 0; q < m; ++q) if (fields[q] == f) return refuse(who, "field %ld is listed twice", f);
        if (!s->lo[f]) return refuse(who, "forced field %ld has no forcing data: icar_hip_forcing_upload comes first", f);
        const FGeoDev &g = f == ICAR_F_U ? s->u : f == ICAR_F_V ? s->v : s->mass;
        if (!g.set) return refuse(who, "field %ld needs the u / v grids' tables, which forcing_configure was not given", f);
        if (f != ICAR_F_U && f != ICAR_F_V && icar_field_count(c, f) != c->n3) return refuse(who, "field %ld is not on the mass grid", f);
        const int *dm = s->lo_dims[f];
        if (dm[0] != g.nx_f || dm[1] != g.nz_f || dm[2] != g.ny_f)
            return refuse(who, "the forcing data of field %ld do not have the extents its look-up tables were made for", f);
        if (f == pressure_field) has_p = true;
    }
    if (has_p) {
        if (pressure_field == ICAR_F_U || pressure_field == ICAR_F_V) return refuse(who, "the pressure is a mass-grid field");
        if (!s->z_f) return refuse(who, "the pressure adjustment needs forcing%%geo%%z and domain%%geo%%z, which forcing_configure was not given");
        if (theta_field < 0 || theta_field >= ICAR_N_FIELD_SLOTS || !s->lo[theta_field])
            return refuse(who, "the pressure adjustment needs the forcing's potential temperature: no forcing data of field %ld", theta_field);
        const int *dm = s->lo_dims[theta_field];
        if (dm[0] != s->mass.nx_f || dm[1] != s->mass.nz_f || dm[2] != s->mass.ny_f) return refuse(who, "the forcing's potential temperature is not on the mass grid's forcing grid");
    }
    return 0;
}

int icar_interpolate_forcing_run(icar_hip_ctx *c, const int *fields, int n, int pressure_field, int theta_field, int update)
{
    if (interpolate_forcing_check(c, "interpolate_forcing", fields, n, pressure_field, theta_field)) return 1;
    ForcingState *s = c->forcing;
    const Dims d = c->d;
    // every destination and temporary exists before the first launch
    float *outs[ICAR_N_FIELD_SLOTS];
    for (int m = 0; m < n; ++m) {
        const int f = fields[m];
        if (!(outs[m] = destination(c, f, update))) return 1;
        if (f == ICAR_F_U || f == ICAR_F_V) {
            const FGeoDev &g = f == ICAR_F_U ? s->u : s->v;
            const size_t ne = (size_t)g.nx * d.nz * g.ny, nl = (size_t)g.nx_f * g.nz_f * g.ny_f;
            if (ensure((void **)&s->ext, s->ext_n, ne, sizeof(float)) || ensure((void **)&s->rowmeans, s->rowmeans_n, ne > nl ? ne : nl, sizeof(double))) return 1;
        } else if (f == pressure_field && !s->p_nv) {
            HIPCHK(hipMalloc(&s->p_nv, c->n3 * sizeof(float))); HIPCHK(hipMalloc(&s->th_nv, c->n3 * sizeof(float)));
        }
    }
    ScopedTimer t(c, "interpolate_forcing");
    const dim3 gcol((d.nx + 63) / 64, d.ny);
    FVars vs; vs.n = 0;
    auto flush = [&]() {
        if (vs.n) { ScopedTimer tm(c, "forcing_mass"); k_forcing_mass<<<gcol, 64, 0, c->stream>>>(geo_arg(s->mass), d.nz, vs); }
        vs.n = 0;
    };
    for (int m = 0; m < n; ++m) {
        const int f = fields[m];
        float *out = outs[m];
        if (!update && icar_field_feeds_winds(f)) icar_winds_changed(c);
        if (f == ICAR_F_U || f == ICAR_F_V) {
            ScopedTimer tw(c, "forcing_wind");
            const FGeoDev &g = f == ICAR_F_U ? s->u : s->v;
            // one grid cell smoothing of the original input data, in place: the forcing's own array changes, as in the reference
            if (smooth_run(c, s, s->lo[f], g.nx_f, g.nz_f, g.ny_f, 1)) return 1;
            FVars one; one.n = 1; one.lo[0] = s->lo[f]; one.out[0] = s->ext;
            k_forcing_mass<<<dim3((g.nx + 63) / 64, g.ny), 64, 0, c->stream>>>(geo_arg(g), d.nz, one);
            if (smooth_run(c, s, s->ext, g.nx, d.nz, g.ny, s->nsmooth)) return 1;
            const int nxd = d.nx + (f == ICAR_F_U), nyd = d.ny + (f == ICAR_F_V);
            k_forcing_box<<<dim3((nxd + 63) / 64, d.nz, nyd), 64, 0, c->stream>>>(s->ext, g.nx, d.nz, g.i0, g.j0, out, nxd, nyd);
        } else if (f == pressure_field) {
            ScopedTimer tp(c, "forcing_pressure");
            FVars two; two.n = 2; two.lo[0] = s->lo[f]; two.out[0] = s->p_nv; two.lo[1] = s->lo[theta_field]; two.out[1] = s->th_nv;
            k_forcing_mass_novert<<<gcol, 64, 0, c->stream>>>(geo_arg(s->mass), d.nz, two);
            k_adjust_pressure<<<gcol, 64, 0, c->stream>>>(d.nx, d.nz, s->mass.nz_f, d.ny, s->p_nv, s->th_nv, s->z_f, s->z_d, out);
        } else {
            vs.lo[vs.n] = s->lo[f]; vs.out[vs.n] = out; ++vs.n;
            if (vs.n == FORCING_MAXV) flush();
        }
    }
    flush();
    HIPCHK(hipGetLastError());
    return 0;
}

int icar_update_delta_fields_run(icar_hip_ctx *c, const int *fields, int n, double dt)
{
    const char *who = "update_delta_fields";
    if (n < 0 || n >= ICAR_N_FIELD_SLOTS) return refuse(who, "bad field count %ld", n);
    if (!(dt > 0.0) || !std::isfinite(dt)) return refuse(who, "dt must be a positive number of seconds");
    FDelta a; int na = 0;
    bool seen[ICAR_N_FIELD_SLOTS] = {false};
    for (int m = 0; m <= n; ++m) {
        const int f = m < n ? fields[m] : ICAR_F_W;             // w is always included, as in the reference (:2368-2369)
        if (f < 0 || f >= ICAR_N_FIELD_SLOTS) return refuse(who, "bad field id %ld", f);
        if (!icar_field_is_3d(c, f)) return refuse(who, "field %ld is 2-D: the dqdt mirrors are 3-D only", f);
        if (seen[f]) { if (m < n && f != ICAR_F_W) return refuse(who, "field %ld is listed twice", f); continue; }
        seen[f] = true;
        if (!c->dqdt[f]) return refuse(who, "field %ld has no dqdt_3d on the device", f);
        if (!c->field[f]) return refuse(who, "field %ld has not been uploaded to the device", f);
        a.dqdt[na] = c->dqdt[f]; a.data[na] = (const float *)c->field[f]; a.n[na] = (unsigned)icar_field_count(c, f); ++na;
    }
    ScopedTimer t(c, "update_delta_fields");
    const unsigned blocks = (unsigned)std::min<size_t>((c->n3 + (size_t)c->d.nz * (c->d.nx + c->d.ny) + 255) / 256, 8192);
    k_update_delta<<<dim3(blocks, na), 256, 0, c->stream>>>(a, dt);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" {

int icar_hip_forcing_configure(icar_hip_ctx *c, const icar_hip_forcing_geo *mass, const icar_hip_forcing_geo *u, const icar_hip_forcing_geo *v,
                               int nsmooth, const float *forcing_z, const float *domain_z, int time_varying_z)
{
    if (icar_enter(c, "forcing_configure")) return 1;
    return forcing_configure_run(c, mass, u, v, nsmooth, forcing_z, domain_z, time_varying_z);
}

int icar_hip_forcing_upload(icar_hip_ctx *c, int field, const float *lo, int nx_f, int nz_f, int ny_f)
{
    if (icar_enter(c, "forcing_upload", lo != nullptr)) return 1;
    return forcing_upload_run(c, field, lo, nx_f, nz_f, ny_f);
}

int icar_hip_forcing_download(icar_hip_ctx *c, int field, float *lo, size_t count)
{
    if (icar_enter(c, "forcing_download", lo != nullptr)) return 1;
    ForcingState *s = c->forcing;
    if (field < 0 || field >= ICAR_N_FIELD_SLOTS || !s || !s->lo[field]) return refuse("forcing_download", "no forcing data of field %ld", field);
    const int *dm = s->lo_dims[field];
    if (count != (size_t)dm[0] * dm[1] * dm[2]) return refuse("forcing_download", "count does not match the %ld elements uploaded", (long)dm[0] * dm[1] * dm[2]);
    HIPCHK(hipMemcpyAsync(lo, s->lo[field], count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_interpolate_forcing(icar_hip_ctx *c, const int *fields, int nfields, int pressure_field, int theta_field, int update)
{
    if (icar_enter(c, "interpolate_forcing", nfields <= 0 || fields)) return 1;
    return icar_interpolate_forcing_run(c, fields, nfields, pressure_field, theta_field, update);
}

int icar_hip_update_delta_fields(icar_hip_ctx *c, const int *fields, int nfields, double dt_seconds)
{
    if (icar_enter(c, "update_delta_fields", nfields <= 0 || fields)) return 1;
    return icar_update_delta_fields_run(c, fields, nfields, dt_seconds);
}

int icar_hip_forcing_step(icar_hip_ctx *c, const int *fields, int nfields, int pressure_field, int theta_field, int windtype, int wind_iterations,
                          float dx, int halo, double dt_seconds)
{
    if (icar_enter(c, "forcing_step", nfields <= 0 || fields)) return 1;
    // what any of the three parts would refuse, before the first launch: a refusal leaves no rate half-made
    const char *who = "forcing_step";
    if (!(dt_seconds > 0.0) || !std::isfinite(dt_seconds)) return refuse(who, "dt must be a positive number of seconds");
    if (wind_iterations < 0 || halo < 1) return refuse(who, "wind_iterations >= 0, halo >= 1");
    if (nfields >= ICAR_N_FIELD_SLOTS) return refuse(who, "bad field count %ld", nfields);
    if (interpolate_forcing_check(c, who, fields, nfields, pressure_field, theta_field)) return 1;
    bool listed[ICAR_N_FIELD_SLOTS] = {false};
    for (int m = 0; m < nfields; ++m) listed[fields[m]] = true;
    for (int f : {ICAR_F_U, ICAR_F_V})
        if (!listed[f] && !c->dqdt[f]) return refuse(who, "update_winds works on the dqdt_3d of u and v: field %ld is neither forced nor has it a dqdt_3d on the device", f);
    for (int m = 0; m <= nfields; ++m) {
        const int f = m < nfields ? fields[m] : ICAR_F_W;
        if (!c->field[f]) return refuse(who, "update_delta_fields needs field %ld on the device: it has not been uploaded", f);
    }
    if (icar_forcing2d_step_check(c, who, dt_seconds)) return 1;                                                   // the enabled 2-D variables (forcing2d.hip)
    for (int m = 0; m <= nfields; ++m) if (!destination(c, m < nfields ? fields[m] : ICAR_F_W, 1)) return 1;      // the mirrors, w's included
    if (icar_interpolate_forcing_run(c, fields, nfields, pressure_field, theta_field, 1)) return 1;
    if (icar_hip_update_winds(c, windtype, wind_iterations, dx, halo, 1)) return 1;
    if (icar_update_delta_fields_run(c, fields, nfields, dt_seconds)) return 1;
    return icar_forcing2d_step_run(c, dt_seconds);
}

}  // extern "C"

// icar_amd/csrc/capi.hip -- extern "C" boundary (include/icar_hip.h), context and field registry, timers.
// The only kernel here is the field fill; every row's kernels live in the file of that row.
#include "ctx.h"
#include "comm.h"
#include <cstring>
#include <cstdio>

static thread_local std::string g_err;
void icar_set_error(const std::string &msg) { g_err = msg; }
int icar_hip_check(hipError_t e, const char *what)
{
    if (e == hipSuccess) return 0;
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return 1;
}

// what every entry point that reaches the device does first: refuse a null context / pointer, select the context's device
// (several contexts, one per device, live in one process)
int icar_enter(icar_hip_ctx *c, const char *who, bool pointers_ok)
{
    if (!c || !pointers_ok) { icar_set_error(std::string(who) + ": null argument"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// field registry
// ------------------------------------------------------------------------------------------------
static bool field_is_2dd(int f) { return icar_field_is_2dd(f); }                   // (ctx.h has the definitions)
static bool field_feeds_winds(int f) { return icar_field_feeds_winds(f); }

size_t icar_field_count(const icar_hip_ctx *c, int f)
{
    const size_t nx = c->d.nx, nz = c->d.nz, ny = c->d.ny;
    if (f == ICAR_F_U || f == ICAR_F_JACOBIAN_U || f == ICAR_F_DZDX || f == ICAR_F_ZR_U) return (nx + 1) * nz * ny;
    if (f == ICAR_F_V || f == ICAR_F_JACOBIAN_V || f == ICAR_F_DZDY || f == ICAR_F_ZR_V) return nx * nz * (ny + 1);
    if (f == ICAR_F_DZ_INTERFACE) return nx * nz * ny;
    if (field_is_2dd(f) || f == ICAR_F_SURFACE_PRESSURE || (f >= ICAR_F_IVT && f <= ICAR_F_IWI) || f >= ICAR_F_TERRAIN) return nx * ny;      // the surface fields of pbl_simple, ra_simple and the surface-flux slot
    return nx * nz * ny;
}

float *icar_field_f(icar_hip_ctx *c, int f, bool required)
{
    if (f < 0 || f >= ICAR_N_FIELD_SLOTS) { icar_set_error("bad field id"); return nullptr; }
    if (!c->field[f]) {
        if (required) {
            char b[96]; snprintf(b, sizeof b, "field %d has not been uploaded to the device", f);
            icar_set_error(b); return nullptr;
        }
        const size_t bytes = icar_field_count(c, f) * icar_hip_field_elem_size(f);
        if (icar_hip_check(hipMalloc(&c->field[f], bytes), "hipMalloc(field)")) return nullptr;
        if (icar_hip_check(hipMemsetAsync(c->field[f], 0, bytes, c->stream), "hipMemset(field)")) return nullptr;
    }
    return (float *)c->field[f];
}

ScopedTimer::ScopedTimer(icar_hip_ctx *c_, const char *g) : c(c_), group(g)
{
    if (!c->timing) return;
    // a timed event pair costs the stream ~5 us (two barrier packets with timestamps); a sub-step of a small tile has a dozen
    // groups: icar_hip_timing_groups restricts the timers to the ones that are read
    if (!c->timing_only.empty() && c->timing_only.find(std::string(",") + g + ",") == std::string::npos) return;
    auto take = [&](hipEvent_t &e) { if (!c->event_pool.empty()) { e = c->event_pool.back(); c->event_pool.pop_back(); } else hipEventCreate(&e); };
    take(e0); take(e1);
    hipEventRecord(e0, c->stream);
}
ScopedTimer::~ScopedTimer()
{
    if (!e0) return;
    hipEventRecord(e1, c->stream);
    c->pending.push_back({group, {e0, e1}});
}

static void drain_timers(icar_hip_ctx *c)
{
    for (auto &p : c->pending) {
        float ms = 0;
        hipEventSynchronize(p.second.second);
        hipEventElapsedTime(&ms, p.second.first, p.second.second);
        auto &t = c->timers[p.first];
        t.total_ms += ms; t.launches += 1;
        c->event_pool.push_back(p.second.first); c->event_pool.push_back(p.second.second);
    }
    c->pending.clear();
}

// icar_hip_field_fill, for REAL(4), REAL(8) and INTEGER(4) fields
template <class T>
__global__ void k_fill(T *p, size_t n, T v) { size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; if (t < n) p[t] = v; }

// ------------------------------------------------------------------------------------------------
// extern "C"
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *icar_hip_last_error(void) { return g_err.c_str(); }
const char *icar_hip_version(void) { return "icar_hip 0.1 (gfx950)"; }
size_t icar_hip_field_elem_size(int field) { return field_is_2dd(field) ? sizeof(double) : sizeof(float); }
size_t icar_hip_field_count(const icar_hip_ctx *ctx, int field) { return ctx ? icar_field_count(ctx, field) : 0; }

int icar_hip_ctx_create(icar_hip_ctx **out, int device, int ims, int ime, int kms, int kme, int jms, int jme)
{
    if (!out) { icar_set_error("ctx_create: null out"); return 1; }
    *out = nullptr;
    if (ime < ims + 2 || jme < jms + 2 || kme < kms + 1) { icar_set_error("ctx_create: tile must be at least 3x2x3"); return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        icar_set_error("ctx_create: no HIP device visible (libicar_hip has no CPU fallback)"); return 1;
    }
    if (device < 0 || device >= ndev) { icar_set_error("ctx_create: bad device index"); return 1; }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950")) {
        icar_set_error(std::string("ctx_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
        return 1;
    }
    icar_hip_ctx *c = new icar_hip_ctx();
    c->device = device;
    c->ims = ims; c->ime = ime; c->kms = kms; c->kme = kme; c->jms = jms; c->jme = jme;
    c->d.nx = ime - ims + 1; c->d.nz = kme - kms + 1; c->d.ny = jme - jms + 1;
    c->d.sk = c->d.nx; c->d.sj = c->d.nx * c->d.nz;
    c->n3 = (size_t)c->d.nx * c->d.nz * c->d.ny;
    if ((size_t)(c->d.nx + 1) * c->d.nz * (c->d.ny + 1) >= (size_t)1 << 31) { delete c; icar_set_error("ctx_create: tile too large for 32-bit indexing"); return 1; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; icar_set_error("hipStreamCreate failed"); return 1; }
    c->own_stream = true;
    if (hipMalloc(&c->d_red, sizeof(float) * (16 + 4096)) != hipSuccess || hipMalloc(&c->d_flag, sizeof(int) * 16) != hipSuccess) {
        delete c; icar_set_error("hipMalloc failed"); return 1;
    }
    *out = c;
    return 0;
}

int icar_hip_ctx_destroy(icar_hip_ctx *c)
{
    if (!c) return 0;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (int f = 0; f < ICAR_N_FIELD_SLOTS; ++f) if (c->field[f]) hipFree(c->field[f]);
    for (int f = 0; f < ICAR_N_ADVECTABLE; ++f) if (c->alt[f]) hipFree(c->alt[f]);
    for (int f = 0; f < ICAR_N_FIELD_SLOTS; ++f) if (c->dqdt[f]) hipFree(c->dqdt[f]);
    float *scr[] = {c->U, c->V, c->W, c->Wdz, c->d_red, c->mpc, c->mpx_buf};
    for (float *p : scr) if (p) hipFree(p);
    if (c->d_flag) hipFree(c->d_flag);
    if (c->h_cfl_pre) hipHostFree(c->h_cfl_pre);
    if (c->cfl_ev) hipEventDestroy(c->cfl_ev);
    if (c->iw_adj) hipFree(c->iw_adj);
    if (c->wgr_tmp) hipFree(c->wgr_tmp);
    if (c->pbl_kq) hipFree(c->pbl_kq);
    if (c->pbl_rowmax) hipFree(c->pbl_rowmax);
    if (c->ra_coslat) hipFree(c->ra_coslat);
    if (c->sfc_levelmax) hipFree(c->sfc_levelmax);
    icar_cu_free(c);
    icar_noah_free(c);
    icar_lsm_driver_free(c);
    icar_ysu_free(c);
    icar_wsm3_free(c);
    icar_wsm6_free(c);
    icar_thompson_free(c);
    icar_linwinds_free(c);
    icar_forcing_free(c);
    icar_forcing2d_free(c);
    icar_comm_free(c);
    if (c->step.h_val) hipHostFree(c->step.h_val);
    if (c->on_aux) c->stream = c->main_saved;
    if (c->aux) { hipStreamSynchronize(c->aux); hipStreamDestroy(c->aux); }
    for (hipEvent_t e : c->event_pool) hipEventDestroy(e);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int icar_hip_set_stream(icar_hip_ctx *c, void *s)
{
    if (!c) { icar_set_error("set_stream: null argument"); return 1; }
    if (c->on_aux) { icar_set_error("set_stream: called between aux_begin and aux_end"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (s) {
        if (c->own_stream) { hipStreamDestroy(c->stream); c->own_stream = false; }
        c->stream = (hipStream_t)s;
    } else if (!c->own_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return 0;
}

int icar_hip_synchronize(icar_hip_ctx *c)
{
    if (icar_enter(c, "synchronize")) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_field_upload(icar_hip_ctx *c, int f, const void *host)
{
    if (icar_enter(c, "field_upload", host != nullptr)) return 1;
    float *p = icar_field_f(c, f, false);
    if (!p) return 1;
    HIPCHK(hipMemcpyAsync(p, host, icar_field_count(c, f) * icar_hip_field_elem_size(f), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (field_feeds_winds(f)) icar_winds_changed(c);
    if (f == ICAR_F_LATITUDE) c->ra_lat_valid = false;
    if (f == ICAR_F_DZ_INTERFACE) c->sfc_nz_valid = false;                        // apply_fluxes looks for nz again
    return 0;
}

int icar_hip_field_download(icar_hip_ctx *c, int f, void *host)
{
    if (icar_enter(c, "field_download", host != nullptr)) return 1;
    float *p = icar_field_f(c, f, true);
    if (!p) return 1;
    HIPCHK(hipMemcpyAsync(host, p, icar_field_count(c, f) * icar_hip_field_elem_size(f), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_field_fill(icar_hip_ctx *c, int f, double value)
{
    if (icar_enter(c, "field_fill")) return 1;
    float *p = icar_field_f(c, f, false);
    if (!p) return 1;
    const size_t n = icar_field_count(c, f);
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    if (field_is_2dd(f))            hipLaunchKernelGGL(k_fill<double>, g, b, 0, c->stream, (double *)p, n, value);
    else if (f == ICAR_F_LAND_MASK) hipLaunchKernelGGL(k_fill<int>, g, b, 0, c->stream, (int *)p, n, (int)value);
    else                            hipLaunchKernelGGL(k_fill<float>, g, b, 0, c->stream, p, n, (float)value);
    HIPCHK(hipGetLastError());
    if (field_feeds_winds(f)) icar_winds_changed(c);
    if (f == ICAR_F_LATITUDE) c->ra_lat_valid = false;
    if (f == ICAR_F_DZ_INTERFACE) c->sfc_nz_valid = false;                        // apply_fluxes looks for nz again
    return 0;
}

int icar_hip_field_device_ptr(icar_hip_ctx *c, int f, void **dptr)
{
    if (icar_enter(c, "field_device_ptr", dptr != nullptr)) return 1;
    float *p = icar_field_f(c, f, false);
    if (!p) return 1;
    *dptr = p;
    if (f == ICAR_F_U || f == ICAR_F_V || f == ICAR_F_W) { c->wind_ptr_escaped = true; icar_winds_changed(c); }   // the caller may write them behind our back
    return 0;
}

int icar_hip_setup_winds(icar_hip_ctx *c, int scheme, float dt, float dx, int advect_density)
{
    if (icar_enter(c, "setup_winds")) return 1;
    return icar_advect_setup_winds(c, scheme, dt, dx, advect_density);
}

int icar_hip_advect(icar_hip_ctx *c, int scheme, int mpdata_order, int fct, int advect_density, const int *fields, int nfields)
{
    if (icar_enter(c, "advect", fields || nfields <= 0)) return 1;
    return icar_advect_run(c, scheme, mpdata_order, fct, advect_density, fields, nfields);
}

int icar_hip_mpdata_exact(icar_hip_ctx *c, int on)
{
    if (!c || (on != 0 && on != 1)) { icar_set_error("mpdata_exact: ctx and on = 0 / 1"); return 1; }
    c->mpdata_exact = on;
    return 0;
}

int icar_hip_mp_simple(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte, int *err_count)
{
    if (icar_enter(c, "mp_simple")) return 1;
    return icar_mp_simple_run(c, dt, its, ite, jts, jte, kts, kte, err_count);
}

int icar_hip_mp_simple_tiles(icar_hip_ctx *c, float dt, int ntiles, const int tiles[][4], int kts, int kte, int *err_count)
{
    if (icar_enter(c, "mp_simple_tiles", tiles != nullptr)) return 1;
    return icar_mp_simple_run_tiles(c, dt, ntiles, tiles, kts, kte, err_count);
}

int icar_hip_thompson_init(icar_hip_ctx *c, const float params[18], const int flags[2])
{
    if (icar_enter(c, "thompson_init", params && flags)) return 1;
    return icar_thompson_init_run(c, params, flags);
}

int icar_hip_thompson(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte,
                      int ids, int ide, int jds, int jde, int kds, int kde)
{
    if (icar_enter(c, "thompson")) return 1;
    return icar_thompson_run(c, dt, its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde);
}

int icar_hip_thompson_tiles(icar_hip_ctx *c, float dt, int ntiles, const int tiles[][4], int kts, int kte,
                            int ids, int ide, int jds, int jde, int kds, int kde)
{
    if (icar_enter(c, "thompson_tiles", tiles != nullptr)) return 1;
    return icar_thompson_run_tiles(c, dt, ntiles, tiles, kts, kte, ids, ide, jds, jde, kds, kde);
}

int icar_hip_thompson_table(icar_hip_ctx *c, const char *name, double *out, size_t capacity, size_t *count)
{
    if (icar_enter(c, "thompson_table", name != nullptr)) return 1;
    return icar_thompson_table_download(c, name, out, capacity, count);
}

int icar_hip_mp_tiles(int its, int ite, int jts, int jte, int halo, int subset, int tiles[4][4])
{
    // mp_driver.f90:609-658 (process_halo) and :728-737 (subset)
    if (halo > 0) {
        const int t[4][4] = {
            {its, its + halo - 1, jts, jte},                     // west strip, full height
            {ite - halo + 1, ite, jts, jte},                     // east strip
            {its + halo, ite - halo, jts, jts + halo - 1},       // south strip without corners
            {its + halo, ite - halo, jte - halo + 1, jte}};      // north strip
        memcpy(tiles, t, sizeof t);
        return 4;
    }
    tiles[0][0] = its + subset; tiles[0][1] = ite - subset; tiles[0][2] = jts + subset; tiles[0][3] = jte - subset;
    return 1;
}

int icar_hip_max_courant(icar_hip_ctx *c, float dx, const float *dz_levels, float *out)
{
    if (icar_enter(c, "max_courant", dz_levels && out)) return 1;
    if (c->d.nz > 4096) { icar_set_error("max_courant: nz too large"); return 1; }
    return icar_max_courant_run(c, dx, dz_levels, out, nullptr);
}

int icar_hip_max_courant_device(icar_hip_ctx *c, float dx, const float *dz_levels, void *d_out)
{
    if (icar_enter(c, "max_courant_device", dz_levels && d_out)) return 1;
    if (c->d.nz > 4096) { icar_set_error("max_courant_device: nz too large"); return 1; }
    return icar_max_courant_run(c, dx, dz_levels, nullptr, (float *)d_out);
}

int icar_hip_max_courant_prefetch(icar_hip_ctx *c, float dx, const float *dz_levels)
{
    if (icar_enter(c, "max_courant_prefetch", dz_levels != nullptr)) return 1;
    if (c->d.nz > 4096) { icar_set_error("max_courant_prefetch: nz too large"); return 1; }
    return icar_max_courant_prefetch_run(c, dx, dz_levels, false);
}

int icar_hip_diagnostic_update(icar_hip_ctx *c)
{
    if (icar_enter(c, "diagnostic_update")) return 1;
    return icar_diagnostic_update_run(c, 3);
}

int icar_hip_diagnostic_update_parts(icar_hip_ctx *c, int parts)
{
    if (!c) { icar_set_error("diagnostic_update_parts: null argument"); return 1; }
    if (parts < 1 || parts > 3) { icar_set_error("diagnostic_update_parts: parts is 1 (thermodynamics), 2 (w_real) or 3"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    return icar_diagnostic_update_run(c, parts);
}

int icar_hip_dqdt_upload(icar_hip_ctx *c, int f, const void *host)
{
    if (icar_enter(c, "dqdt_upload", host != nullptr)) return 1;
    if (f < 0 || f >= ICAR_N_FIELD_SLOTS || field_is_2dd(f) || f >= ICAR_F_TERRAIN) { icar_set_error("dqdt_upload: bad field"); return 1; }
    const size_t bytes = icar_field_count(c, f) * sizeof(float);
    if (!c->dqdt[f]) HIPCHK(hipMalloc(&c->dqdt[f], bytes));
    HIPCHK(hipMemcpyAsync(c->dqdt[f], host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_apply_forcing(icar_hip_ctx *c, double dt, const int *fields, const int *fb, int n, int w, int e, int s, int nn)
{
    if (icar_enter(c, "apply_forcing", n <= 0 || (fields && fb))) return 1;
    return icar_apply_forcing_run(c, dt, fields, fb, n, w, e, s, nn);
}

int icar_hip_enforce_limits(icar_hip_ctx *c, const int *fields, int n)
{
    if (icar_enter(c, "enforce_limits", n <= 0 || fields)) return 1;
    return icar_enforce_limits_run(c, fields, n);
}

int icar_hip_wsm6_tiles(icar_hip_ctx *c, float dt, int ntiles, const int tiles[][4], int kts, int kte)
{
    if (icar_enter(c, "wsm6_tiles", tiles != nullptr)) return 1;
    return icar_wsm6_run_tiles(c, dt, ntiles, tiles, kts, kte);
}

int icar_hip_winds_valid(icar_hip_ctx *c) { return (c && c->winds_valid) ? 1 : 0; }

int icar_hip_pbl_simple(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    if (icar_enter(c, "pbl_simple")) return 1;
    return icar_pbl_simple_run(c, dt, its, ite, jts, jte, kts, kte);
}

int icar_hip_ra_simple(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte, int runlw)
{
    if (icar_enter(c, "ra_simple")) return 1;
    double D, year_days;
    if (icar_rad_clock(c, c->step.model_time, &D, &year_days)) return 1;
    return icar_ra_simple_run(c, dt, its, ite, jts, jte, kts, kte, runlw, c->step.rad_calendar, D, year_days);
}

int icar_hip_pbl_nsubsteps(icar_hip_ctx *c, int *nsubsteps, int nrows)
{
    if (icar_enter(c, "pbl_nsubsteps", nsubsteps != nullptr)) return 1;
    return icar_pbl_nsubsteps_copy(c, nsubsteps, nrows);
}

int icar_hip_wsm6_init(icar_hip_ctx *c)
{
    if (icar_enter(c, "wsm6_init")) return 1;
    return icar_wsm6_init_run(c);
}

int icar_hip_wsm6(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    if (icar_enter(c, "wsm6")) return 1;
    return icar_wsm6_run(c, dt, its, ite, jts, jte, kts, kte);
}

int icar_hip_wsm3_init(icar_hip_ctx *c)
{
    if (icar_enter(c, "wsm3_init")) return 1;
    return icar_wsm3_init_run(c);
}

int icar_hip_wsm3(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte)
{
    if (icar_enter(c, "wsm3")) return 1;
    return icar_wsm3_run(c, dt, its, ite, jts, jte, kts, kte);
}

int icar_hip_max_abs_winds(icar_hip_ctx *c, float *out3)
{
    if (icar_enter(c, "max_abs_winds", out3 != nullptr)) return 1;
    return icar_max_abs_winds_run(c, out3);
}

int icar_hip_balance_uvw(icar_hip_ctx *c, float dx)
{
    if (icar_enter(c, "balance_uvw")) return 1;
    return icar_balance_uvw_run(c, dx, 0);
}

int icar_hip_balance_uvw_update(icar_hip_ctx *c, float dx)
{
    if (icar_enter(c, "balance_uvw_update")) return 1;
    return icar_balance_uvw_run(c, dx, 1);
}

int icar_hip_make_winds_grid_relative(icar_hip_ctx *c, int update)
{
    if (icar_enter(c, "make_winds_grid_relative")) return 1;
    return icar_make_winds_grid_relative(c, update);
}

int icar_hip_mass_conservative_acceleration(icar_hip_ctx *c, int update)
{
    if (icar_enter(c, "mass_conservative_acceleration")) return 1;
    return icar_mass_conservative_acceleration(c, update);
}

int icar_hip_iterative_winds_correct_w(icar_hip_ctx *c, int update)
{
    if (icar_enter(c, "iterative_winds_correct_w")) return 1;
    return icar_iterative_winds_correct_w(c, update);
}

int icar_hip_iterative_winds_sweep(icar_hip_ctx *c, float dx, int nsweeps, int update)
{
    if (icar_enter(c, "iterative_winds_sweep")) return 1;
    if (nsweeps < 0 || !(dx > 0)) { icar_set_error("iterative_winds_sweep: bad argument"); return 1; }
    return icar_iterative_winds_sweep(c, dx, nsweeps, update);
}

int icar_hip_box_pack(icar_hip_ctx *c, int field, int which, int i0, int ni, int j0, int nj, void *dbuf)
{
    if (icar_enter(c, "box_pack", dbuf != nullptr)) return 1;
    return icar_box_copy(c, field, which, i0, ni, j0, nj, (float *)dbuf, false);
}

int icar_hip_box_unpack(icar_hip_ctx *c, int field, int which, int i0, int ni, int j0, int nj, const void *dbuf)
{
    if (icar_enter(c, "box_unpack", dbuf != nullptr)) return 1;
    if (which == 0 && (field == ICAR_F_U || field == ICAR_F_V || field == ICAR_F_W)) icar_winds_changed(c);
    return icar_box_copy(c, field, which, i0, ni, j0, nj, (float *)dbuf, true);
}

int icar_hip_dqdt_download(icar_hip_ctx *c, int f, void *host)
{
    if (icar_enter(c, "dqdt_download", host != nullptr)) return 1;
    if (f < 0 || f >= ICAR_N_FIELD_SLOTS || field_is_2dd(f) || !c->dqdt[f]) { icar_set_error("dqdt_download: no dqdt mirror for this field"); return 1; }
    HIPCHK(hipMemcpyAsync(host, c->dqdt[f], icar_field_count(c, f) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int icar_hip_linwinds_setup(icar_hip_ctx *c, const icar_hip_lt_options *opt, const float *global_terrain,
                            int nx_global, int ny_global, int ids, int jds, float dx)
{
    if (!c || !opt || !global_terrain) { icar_set_error("linwinds_setup: null argument"); return 1; }
    if (nx_global < 2 || ny_global < 2 || !(dx > 0)) { icar_set_error("linwinds_setup: bad global terrain size / dx"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    return icar_linwinds_setup_run(c, opt, global_terrain, nx_global, ny_global, ids, jds, dx);
}

int icar_hip_linwinds_terrain_frequency(icar_hip_ctx *c, double *out, size_t cap, int *fftnx, int *fftny)
{
    if (icar_enter(c, "linwinds_terrain_frequency")) return 1;
    return icar_linwinds_terrain_frequency(c, out, cap, fftnx, fftny);
}

int icar_hip_linear_perturbation(icar_hip_ctx *c, float U, float V, float Nsq, float z_bottom, float z_top,
                                 float minimum_step, double *u_perturb, double *v_perturb)
{
    if (!c || !u_perturb || !v_perturb) { icar_set_error("linear_perturbation: null argument"); return 1; }
    if (!(minimum_step > 0) || !(z_top > z_bottom)) { icar_set_error("linear_perturbation: need z_top > z_bottom and minimum_step > 0"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    return icar_linear_perturbation_run(c, U, V, Nsq, z_bottom, z_top, minimum_step, u_perturb, v_perturb);
}

int icar_hip_linwinds_build_lut(icar_hip_ctx *c, const float *z_bottom, const float *z_top, int nz)
{
    if (!c || !z_bottom || !z_top) { icar_set_error("linwinds_build_lut: null argument"); return 1; }
    for (int k = 0; k < nz; ++k) if (!(z_top[k] > z_bottom[k])) { icar_set_error("linwinds_build_lut: need z_top > z_bottom on every level"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    return icar_linwinds_build_lut_run(c, z_bottom, z_top, nz);
}

int icar_hip_linwinds_build_lut_varying(icar_hip_ctx *c, const float *z_bottom, const float *z_top, int nz)
{
    if (icar_enter(c, "linwinds_build_lut_varying", z_bottom && z_top)) return 1;
    return icar_linwinds_build_lut_varying_run(c, z_bottom, z_top, nz);
}

int icar_hip_linwinds_lut_download(icar_hip_ctx *c, int comp, float *host)
{
    if (icar_enter(c, "linwinds_lut_download", host != nullptr)) return 1;
    return icar_linwinds_lut_copy(c, comp, host, 0);
}

int icar_hip_linwinds_lut_entry(icar_hip_ctx *c, int comp, int spd, int dir, int nsq, float *host)
{
    if (icar_enter(c, "linwinds_lut_entry", host != nullptr)) return 1;
    return icar_linwinds_lut_entry(c, comp, spd, dir, nsq, host);
}

int icar_hip_linwinds_lut_upload(icar_hip_ctx *c, int comp, const float *host)
{
    if (icar_enter(c, "linwinds_lut_upload", host != nullptr)) return 1;
    return icar_linwinds_lut_copy(c, comp, const_cast<float *>(host), 1);
}

int icar_hip_linwinds_perturbation_download(icar_hip_ctx *c, int comp, float *host)
{
    if (icar_enter(c, "linwinds_perturbation_download", host != nullptr)) return 1;
    return icar_linwinds_pert_copy(c, comp, host, 0);
}

int icar_hip_linwinds_perturbation_upload(icar_hip_ctx *c, int comp, const float *host)
{
    if (icar_enter(c, "linwinds_perturbation_upload", host != nullptr)) return 1;
    return icar_linwinds_pert_copy(c, comp, const_cast<float *>(host), 1);
}

int icar_hip_spatial_winds(icar_hip_ctx *c, int update)
{
    if (icar_enter(c, "spatial_winds")) return 1;
    return icar_spatial_winds_run(c, update);
}

size_t icar_hip_halo_count(const icar_hip_ctx *c, int dir, int halo)
{
    if (!c) return 0;
    if (dir == 0 || dir == 1) return (size_t)c->d.nx * c->d.nz * halo;
    return (size_t)halo * c->d.nz * c->d.ny;
}

int icar_hip_halo_pack(icar_hip_ctx *c, int dir, int halo, const int *fields, int nfields, void *dbuf)
{
    if (icar_enter(c, "halo_pack", dbuf != nullptr)) return 1;
    return icar_halo_pack_dirs(c, 1, &dir, halo, fields, nfields, &dbuf, false);
}

int icar_hip_halo_pack_dirs(icar_hip_ctx *c, int ndir, const int *dirs, int halo, const int *fields, int nfields, void *const *dbufs)
{
    if (icar_enter(c, "halo_pack_dirs", dirs && dbufs)) return 1;
    return icar_halo_pack_dirs(c, ndir, dirs, halo, fields, nfields, dbufs, false);
}

int icar_hip_halo_unpack_dirs(icar_hip_ctx *c, int ndir, const int *dirs, int halo, const int *fields, int nfields, void *const *dbufs)
{
    if (icar_enter(c, "halo_unpack_dirs", dirs && dbufs)) return 1;
    return icar_halo_pack_dirs(c, ndir, dirs, halo, fields, nfields, dbufs, true);
}

int icar_hip_halo_unpack(icar_hip_ctx *c, int dir, int halo, const int *fields, int nfields, const void *dbuf)
{
    if (icar_enter(c, "halo_unpack", dbuf != nullptr)) return 1;
    void *buf = const_cast<void *>(dbuf);
    return icar_halo_pack_dirs(c, 1, &dir, halo, fields, nfields, &buf, true);
}

// ---- second stream -------------------------------------------------------------------------------------------------
// aux_fork : the aux stream waits for everything issued on the main stream so far
// aux_begin / aux_end : entry points called in between launch on the aux stream
// aux_join : the main stream waits for everything issued on the aux stream so far
static int ensure_aux(icar_hip_ctx *c)
{
    if (c->aux) return 0;
    // same priority as the main stream: the strips are issued first and start first; a lowest-priority aux stream measured
    // 1.5 % slower per step (the interior launch is the bulk of the step's work and must not be throttled)
    HIPCHK(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    return 0;
}

int icar_hip_aux_fork(icar_hip_ctx *c)
{
    if (!c) { icar_set_error("aux_fork: null argument"); return 1; }
    if (c->on_aux) { icar_set_error("aux_fork: already on the aux stream"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    if (ensure_aux(c)) return 1;
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    return 0;
}

int icar_hip_aux_begin(icar_hip_ctx *c)
{
    if (!c) { icar_set_error("aux_begin: null argument"); return 1; }
    if (c->on_aux) { icar_set_error("aux_begin: already on the aux stream"); return 1; }
    HIPCHK(hipSetDevice(c->device));
    if (ensure_aux(c)) return 1;
    c->main_saved = c->stream; c->stream = c->aux; c->on_aux = true;
    return 0;
}

int icar_hip_aux_end(icar_hip_ctx *c)
{
    if (!c) { icar_set_error("aux_end: null argument"); return 1; }
    if (!c->on_aux) { icar_set_error("aux_end: not on the aux stream"); return 1; }
    c->stream = c->main_saved; c->on_aux = false;
    return 0;
}

int icar_hip_aux_join(icar_hip_ctx *c)
{
    if (!c) { icar_set_error("aux_join: null argument"); return 1; }
    if (c->on_aux) { icar_set_error("aux_join: call aux_end first"); return 1; }
    if (!c->aux) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev_join, c->aux));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return 0;
}

int icar_hip_timing_enable(icar_hip_ctx *c, int on) { if (icar_enter(c, "timing_enable")) return 1; c->timing = on != 0; return 0; }
int icar_hip_timing_groups(icar_hip_ctx *c, const char *csv)
{
    if (!c) return 1;
    c->timing_only = (csv && *csv) ? std::string(",") + csv + "," : std::string();
    return 0;
}
int icar_hip_timing_reset(icar_hip_ctx *c) { if (icar_enter(c, "timing_reset")) return 1; hipStreamSynchronize(c->stream); drain_timers(c); c->timers.clear(); return 0; }
int icar_hip_timing_read(icar_hip_ctx *c, const char *group, double *total_ms, int *launches)
{
    if (icar_enter(c, "timing_read", group != nullptr)) return 1;
    hipStreamSynchronize(c->stream);
    drain_timers(c);
    auto it = c->timers.find(group);
    if (total_ms) *total_ms = (it == c->timers.end()) ? 0.0 : it->second.total_ms;
    if (launches) *launches = (it == c->timers.end()) ? 0 : it->second.launches;
    return 0;
}

}  // extern "C"

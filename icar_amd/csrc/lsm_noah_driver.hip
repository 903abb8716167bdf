// icar_amd/csrc/lsm_noah_driver.hip -- the Noah branch of lsm() around the call of lsm_noah on gfx950 (landsurface = kLSM_NOAH = 3), and
// what lsm_init does for it beside the Noah part that lsm_noah.hip holds.
//
// Reference algorithm: src/physics/lsm_driver.f90 -- lsm_init :566 (Z0), :583-587, :592-596 (CHS, CHS2), :602-603 (RAINBL), :610-611
// (temperature_2m, humidity_2m), :992-997 (z_atm, lnz_atm_term, base_exchange_term); lsm :1028-1030 with calc_exchange_coefficient
// :244-265, :1144-1147 (CHS times the floored wind speed, copied to CHS2 and CQS2), :1181-1187 (QGH), :1207 (current_precipitation),
// :1280-1290 (max_swe, the exchange terms from the new roughness_z0, longwave_up, RAINBL), :1524-1527 (soil_totalmoisture),
// surface_diagnostics :299-359 (the bulk arm).  The cell code is lsm_noah_driver_cell.h, which also says what is not built and why.
//
//   k_lsm_noah_couple  one thread per (i,j) of the memory rectangle: lsm_init's statements above
//   k_lsm_noah_pre     one thread per (i,j) of the memory rectangle, ahead of water_simple and k_noah: windspd, Ri, CHS (= CHS2 = CQS2),
//                      QGH where land_mask == kLC_LAND, current_precipitation.  water_simple reads nothing this kernel writes and writes
//                      skin_temperature, which Ri reads as it was: hence ahead of it, in the reference's order
//   k_lsm_noah_post    one thread per (i,j) of the memory rectangle, behind k_noah: the max_swe clamp, the exchange terms, longwave_up,
//                      RAINBL, soil_totalmoisture; and on its..ite, jts..jte the 2 m diagnostics
// k_noah (lsm_noah.hip) runs unchanged between the two: it sits at the register limit without scratch and takes nothing more.
// Lanes along i, no LDS, no barrier; REAL(4) loads and stores are raw buffer accesses with a wave-uniform row offset; the two REAL(8)
// arrays (accumulated_precipitation, RAINBL) are plain global accesses.  No contraction, IEEE division and square root; logf / expf are
// glibc's (glibc_flt32.h).
#include "ctx.h"
#include "glibc_flt32.h"
#include <cstdio>
#include <string>

#define LND_FN __device__ static __forceinline__
#define LND_LOGF gf_logf
#define LND_EXPF gf_expf
#define LND_SQRTF sqrtf
#include "lsm_noah_driver_cell.h"

// the ICAR_LSM_* arrays: RAINBL (REAL(8)) first, then the six REAL(4) planes, in one allocation
struct LsmDriverState {
    double *rainbl = nullptr;
    float *arr[ICAR_LSM_N] = {nullptr};      // (ICAR_LSM_RAINBL's entry is rainbl)
    bool coupled = false;
};

namespace {
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t mk(const void *p) { return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, -1, 0x00020000); }
__device__ __forceinline__ float ld(const void *p, int voff, int soff) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mk(p), voff, soff, 0)); }
__device__ __forceinline__ int ldi(const void *p, int voff, int soff) { return __builtin_amdgcn_raw_buffer_load_b32(mk(p), voff, soff, 0); }
__device__ __forceinline__ void st(float x, void *p, int voff, int soff) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, x), mk(p), voff, soff, 0); }

struct CoupleArgs {
    Dims d;
    const float *z0, *z, *terrain, *temperature, *qv;
    const double *precip;
    float *noah_z0, *chs, *chs2, *curprecip, *t2, *q2, *z_atm, *lnz, *base;
    double *rainbl;
};

__global__ void __launch_bounds__(64)
k_lsm_noah_couple(CoupleArgs a)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= a.d.nx) return;
    const int vi = 4 * i, s2 = 4 * a.d.nx * j, s3 = 4 * a.d.idx(0, 0, j);        // level kms = kts
    const size_t at = (size_t)a.d.nx * j + i;
    const float z0 = ld(a.z0, vi, s2);
    const float z_atm = ld(a.z, vi, s3) - ld(a.terrain, vi, s2);                 // :992
    float lnz, base;
    lnd_exchange_terms(z_atm, z0, &lnz, &base);                                  // :993-996
    st(z0, a.noah_z0, vi, s2);                                                   // :566
    st(0.01f, a.chs, vi, s2);                                                    // :593
    st(0.01f, a.chs2, vi, s2);                                                   // :596
    st(0.0f, a.curprecip, vi, s2);                                               // :584
    a.rainbl[at] = a.precip[at];                                                 // :603
    st(ld(a.temperature, vi, s3), a.t2, vi, s2);                                 // :610
    st(ld(a.qv, vi, s3), a.q2, vi, s2);                                          // :611
    st(z_atm, a.z_atm, vi, s2);
    st(lnz, a.lnz, vi, s2);
    st(base, a.base, vi, s2);
}

struct PreArgs {
    Dims d;
    const float *u10, *v10, *tskin, *temperature, *z_atm, *lnz, *base, *t2, *psfc;
    const int *land_mask;
    const double *precip, *rainbl;
    float *ri, *chs, *chs2, *cqs2, *qgh, *curprecip;
};

__global__ void __launch_bounds__(64)
k_lsm_noah_pre(PreArgs a)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= a.d.nx) return;
    const int vi = 4 * i, s2 = 4 * a.d.nx * j, s3 = 4 * a.d.idx(0, 0, j);        // airt(:,1,:): the first level of the memory
    const size_t at = (size_t)a.d.nx * j + i;
    float ri, chs;
    int flags;
    lnd_exchange(ld(a.u10, vi, s2), ld(a.v10, vi, s2), ld(a.tskin, vi, s2), ld(a.temperature, vi, s3), ld(a.z_atm, vi, s2), ld(a.lnz, vi, s2),
                 ld(a.base, vi, s2), &ri, &chs, &flags);
    st(ri, a.ri, vi, s2);
    st(chs, a.chs, vi, s2);                                                      // :1145
    st(chs, a.chs2, vi, s2);                                                     // :1146
    st(chs, a.cqs2, vi, s2);                                                     // :1147
    if (ldi(a.land_mask, vi, s2) == LND_LC_LAND) st(lnd_sat_mr(ld(a.t2, vi, s2), ld(a.psfc, vi, s2)), a.qgh, vi, s2);   // :1181-1187
    st(lnd_current_precipitation(a.precip[at], a.rainbl[at]), a.curprecip, vi, s2);                                    // :1207
}

struct PostArgs {
    Dims d;
    int i0, i1, j0, j1;                      // the tile, 0-based inclusive
    float max_swe;
    const float *z_atm, *znt, *emiss, *tskin, *smois, *hfx, *qfx, *qsfc, *chs2, *cqs2, *psfc;
    const double *precip;
    float *swe, *lnz, *base, *lwup, *smstot, *t2, *q2;
    double *rainbl;
};

__global__ void __launch_bounds__(64)
k_lsm_noah_post(PostArgs a)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (i >= a.d.nx) return;
    const int vi = 4 * i, s2 = 4 * a.d.nx * j, ss = 4 * a.d.nx * 4 * j, sl = 4 * a.d.nx;   // the soil arrays are (nx, 4, ny)
    const size_t at = (size_t)a.d.nx * j + i;
    st(lnd_max_swe(ld(a.swe, vi, s2), a.max_swe), a.swe, vi, s2);                // :1280
    float lnz, base;
    lnd_exchange_terms(ld(a.z_atm, vi, s2), ld(a.znt, vi, s2), &lnz, &base);     // :1282-1285
    st(lnz, a.lnz, vi, s2);
    st(base, a.base, vi, s2);
    const float tsk = ld(a.tskin, vi, s2);
    st(lnd_longwave_up(ld(a.emiss, vi, s2), tsk), a.lwup, vi, s2);               // :1289
    a.rainbl[at] = a.precip[at];                                                 // :1290
    st(lnd_soil_totalmoisture(ld(a.smois, vi, ss), ld(a.smois, vi, ss + sl), ld(a.smois, vi, ss + 2 * sl), ld(a.smois, vi, ss + 3 * sl)), a.smstot, vi, s2);   // :1524-1527
    if (i < a.i0 || i > a.i1 || j < a.j0 || j > a.j1) return;
    float t2, q2;
    int flags;
    lnd_surface_diagnostics(ld(a.hfx, vi, s2), ld(a.qfx, vi, s2), tsk, ld(a.qsfc, vi, s2), ld(a.chs2, vi, s2), ld(a.cqs2, vi, s2), ld(a.psfc, vi, s2),
                            &t2, &q2, &flags);                                   // :1530-1545
    st(t2, a.t2, vi, s2);
    st(q2, a.q2, vi, s2);
}

struct Need { int f; const char *member; };

// every field of `list` is on the device, or the error names the first that is not
bool fields_there(icar_hip_ctx *c, const char *who, const Need *list, int n)
{
    for (int k = 0; k < n; ++k)
        if (!c->field[list[k].f]) {
            char b[200]; snprintf(b, sizeof b, "%s: domain%%%s (field %d) is not on the device", who, list[k].member, list[k].f);
            icar_set_error(b); return false;
        }
    return true;
}

bool limits_ok(icar_hip_ctx *c, const char *who)
{
    if (c->n3 * sizeof(float) >= ((size_t)1 << 31)) { icar_set_error(std::string(who) + ": a field of 2 GiB or more is not supported (32-bit offsets)"); return false; }
    if ((size_t)c->d.nx * c->d.ny * 4 * sizeof(float) >= ((size_t)1 << 31)) { icar_set_error(std::string(who) + ": a soil array of 2 GiB or more is not supported (32-bit offsets)"); return false; }
    if (c->d.ny > 65535) { icar_set_error(std::string(who) + ": more than 65535 rows are not supported"); return false; }
    return true;
}

bool level_ok(icar_hip_ctx *c, const char *who)
{
    const int kts = c->step.configured ? c->step.cfg.kts : c->kms;
    if (kts == c->kms && kts == 1 && c->kme >= 2) return true;
    icar_set_error(std::string(who) + ": a step tile with kts /= kms: lsm_noah names level 1 literally and lsm() reads airt(:,1,:) beside z(:,kts,:) "
                   "(lsm_driver.f90:254, :992): only kts = kms = 1 with at least two levels is built");
    return false;
}

int arrays(icar_hip_ctx *c)
{
    if (!c->lsmdrv) c->lsmdrv = new LsmDriverState();
    LsmDriverState *s = c->lsmdrv;
    if (s->rainbl) return 0;
    const size_t n2 = (size_t)c->d.nx * c->d.ny, bytes = n2 * (sizeof(double) + (ICAR_LSM_N - 1) * sizeof(float));
    HIPCHK(hipMalloc(&s->rainbl, bytes));
    HIPCHK(hipMemsetAsync(s->rainbl, 0, bytes, c->stream));
    float *p = (float *)(s->rainbl + n2);
    for (int w = 0; w < ICAR_LSM_N; ++w) {
        if (w == ICAR_LSM_RAINBL) s->arr[w] = (float *)s->rainbl;
        else { s->arr[w] = p; p += n2; }
    }
    return 0;
}

int lsm_copy(icar_hip_ctx *c, const char *who, int which, void *host, bool to_device)
{
    if (which < 0 || which >= ICAR_LSM_N) { icar_set_error(std::string(who) + ": `which` is one of ICAR_LSM_* (enum icar_hip_lsm_array)"); return 1; }
    if (arrays(c)) return 1;
    const size_t bytes = (size_t)c->d.nx * c->d.ny * (which == ICAR_LSM_RAINBL ? sizeof(double) : sizeof(float));
    void *dev = c->lsmdrv->arr[which];
    if (to_device) HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace

void icar_lsm_driver_free(icar_hip_ctx *c)
{
    if (!c->lsmdrv) return;
    if (c->lsmdrv->rainbl) hipFree(c->lsmdrv->rainbl);
    delete c->lsmdrv;
    c->lsmdrv = nullptr;
}

void icar_lsm_uncouple(icar_hip_ctx *c) { if (c->lsmdrv) c->lsmdrv->coupled = false; }
bool icar_lsm_noah_coupled(const icar_hip_ctx *c) { return c->lsmdrv && c->lsmdrv->coupled && icar_noah_ready(c) && c->step.landsurface == ICAR_LSM_NOAH; }

extern "C" int icar_hip_lsm_upload(icar_hip_ctx *c, int which, const void *host)
{
    if (icar_enter(c, "lsm_upload", host != nullptr)) return 1;
    return lsm_copy(c, "lsm_upload", which, const_cast<void *>(host), true);
}

extern "C" int icar_hip_lsm_download(icar_hip_ctx *c, int which, void *host)
{
    if (icar_enter(c, "lsm_download", host != nullptr)) return 1;
    return lsm_copy(c, "lsm_download", which, host, false);
}

// what lsm_init does for Noah beside icar_hip_lsm_init's part; from here on icar_hip_lsm and the step entry points run the Noah branch
extern "C" int icar_hip_lsm_noah_couple(icar_hip_ctx *c)
{
    static const char *who = "lsm_noah_couple";
    if (icar_enter(c, who)) return 1;
    if (!icar_noah_ready(c) || c->step.landsurface != ICAR_LSM_NOAH) {
        icar_set_error(std::string(who) + ": Noah is not initialised (icar_hip_noah_tables, the ICAR_NOAH_* arrays and icar_hip_lsm_init with landsurface = 3 "
                       "come first, and again after new tables, new veg_type / soil_type or another icar_hip_lsm_init / icar_hip_lsm_configure)");
        return 1;
    }
    if (!level_ok(c, who)) return 1;
    static const Need must[] = {{ICAR_F_ROUGHNESS_Z0, "roughness_z0"}, {ICAR_F_Z, "z"}, {ICAR_F_TERRAIN, "terrain"}, {ICAR_F_TEMPERATURE, "temperature"},
                                {ICAR_F_WATER_VAPOR, "water_vapor"}, {ICAR_F_SURFACE_PRESSURE, "surface_pressure"}};
    if (!fields_there(c, who, must, 6)) return 1;
    // the 10 m winds: there already, or icar_hip_diag_10m's inputs are (then every lsm() finds what the step's diagnostic_update made)
    if (!c->field[ICAR_F_U_10M] || !c->field[ICAR_F_V_10M]) {
        static const Need winds[] = {{ICAR_F_U_MASS, "u_mass (for u_10m / v_10m, which are not there either)"}, {ICAR_F_V_MASS, "v_mass (for u_10m / v_10m, which are not there either)"}};
        if (!fields_there(c, who, winds, 2)) return 1;
    }
    if (!limits_ok(c, who)) return 1;
    // the last refusal: from here on the state is written.  accumulated_precipitation never uploaded is the zeros domain_t allocates
    if (arrays(c)) return 1;
    LsmDriverState *s = c->lsmdrv;
    const double *precip = (const double *)icar_field_f(c, ICAR_F_PRECIPITATION, false);
    if (!precip) return 1;
    if (!c->field[ICAR_F_U_10M] || !c->field[ICAR_F_V_10M]) { if (icar_sfc_diag_10m_run(c)) return 1; }
    CoupleArgs a;
    a.d = c->d;
    a.z0 = (const float *)c->field[ICAR_F_ROUGHNESS_Z0]; a.z = (const float *)c->field[ICAR_F_Z]; a.terrain = (const float *)c->field[ICAR_F_TERRAIN];
    a.temperature = (const float *)c->field[ICAR_F_TEMPERATURE]; a.qv = (const float *)c->field[ICAR_F_WATER_VAPOR]; a.precip = precip;
    a.noah_z0 = icar_noah_array(c, ICAR_NOAH_Z0); a.chs = icar_noah_array(c, ICAR_NOAH_CHS); a.chs2 = icar_noah_array(c, ICAR_NOAH_CHS2);
    a.curprecip = icar_noah_array(c, ICAR_NOAH_CURRENT_PRECIPITATION);
    a.t2 = s->arr[ICAR_LSM_TEMPERATURE_2M]; a.q2 = s->arr[ICAR_LSM_HUMIDITY_2M]; a.z_atm = s->arr[ICAR_LSM_Z_ATM]; a.lnz = s->arr[ICAR_LSM_LNZ_ATM_TERM];
    a.base = s->arr[ICAR_LSM_BASE_EXCHANGE_TERM]; a.rainbl = s->rainbl;
    hipLaunchKernelGGL(k_lsm_noah_couple, dim3((c->d.nx + 63) / 64, c->d.ny), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    s->coupled = true;
    return 0;
}

// the gated block of lsm() for kLSM_NOAH on the tile of icar_hip_step_configure (sfc_basic.hip: icar_lsm_run holds the gate and calls
// apply_fluxes behind it).  Everything that can be refused is looked at before the first launch.
int icar_lsm_noah_gated_run(icar_hip_ctx *c, float lsm_dt)
{
    static const char *who = "lsm";
    LsmDriverState *s = c->lsmdrv;
    const icar_hip_step_config &g = c->step.cfg;
    if (!level_ok(c, who) || !limits_ok(c, who)) return 1;
    static const Need must[] = {{ICAR_F_U_10M, "u_10m"}, {ICAR_F_V_10M, "v_10m"}, {ICAR_F_SKIN_TEMPERATURE, "skin_temperature"}, {ICAR_F_TEMPERATURE, "temperature"},
                                {ICAR_F_SURFACE_PRESSURE, "surface_pressure"}, {ICAR_F_LAND_MASK, "land_mask"}, {ICAR_F_PRECIPITATION, "accumulated_precipitation"},
                                {ICAR_F_WATER_VAPOR, "water_vapor"}, {ICAR_F_PRESSURE_INTERFACE, "pressure_interface"}, {ICAR_F_SHORTWAVE, "shortwave"},
                                {ICAR_F_LONGWAVE, "longwave"}, {ICAR_F_SENSIBLE_HEAT, "sensible_heat"}, {ICAR_F_LATENT_HEAT, "latent_heat"},
                                {ICAR_F_ROUGHNESS_Z0, "roughness_z0"}};
    if (!fields_there(c, who, must, sizeof must / sizeof must[0])) return 1;
    if (c->step.watersurface == ICAR_WATER_SIMPLE) {
        static const Need water[] = {{ICAR_F_USTAR, "ustar"}, {ICAR_F_SST, "sst"}, {ICAR_F_Z, "z"}, {ICAR_F_TERRAIN, "terrain"}};
        if (!fields_there(c, "water_simple", water, 4)) return 1;
    }
    if (g.its < c->ims || g.ite > c->ime || g.jts < c->jms || g.jte > c->jme) { icar_set_error("lsm: tile outside memory bounds"); return 1; }
    const dim3 grid((c->d.nx + 63) / 64, c->d.ny), block(64);
    {
        PreArgs a;
        a.d = c->d;
        a.u10 = (const float *)c->field[ICAR_F_U_10M]; a.v10 = (const float *)c->field[ICAR_F_V_10M]; a.tskin = (const float *)c->field[ICAR_F_SKIN_TEMPERATURE];
        a.temperature = (const float *)c->field[ICAR_F_TEMPERATURE]; a.psfc = (const float *)c->field[ICAR_F_SURFACE_PRESSURE];
        a.land_mask = (const int *)c->field[ICAR_F_LAND_MASK]; a.precip = (const double *)c->field[ICAR_F_PRECIPITATION]; a.rainbl = s->rainbl;
        a.z_atm = s->arr[ICAR_LSM_Z_ATM]; a.lnz = s->arr[ICAR_LSM_LNZ_ATM_TERM]; a.base = s->arr[ICAR_LSM_BASE_EXCHANGE_TERM]; a.t2 = s->arr[ICAR_LSM_TEMPERATURE_2M];
        a.ri = icar_noah_array(c, ICAR_NOAH_RI); a.chs = icar_noah_array(c, ICAR_NOAH_CHS); a.chs2 = icar_noah_array(c, ICAR_NOAH_CHS2);
        a.cqs2 = icar_noah_array(c, ICAR_NOAH_CQS2); a.qgh = icar_noah_array(c, ICAR_NOAH_QGH); a.curprecip = icar_noah_array(c, ICAR_NOAH_CURRENT_PRECIPITATION);
        ScopedTimer timer(c, "lsm_noah_pre");
        hipLaunchKernelGGL(k_lsm_noah_pre, grid, block, 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (c->step.watersurface == ICAR_WATER_SIMPLE && icar_sfc_water_simple_run(c)) return 1;           // :1051-1073
    if (icar_noah_run(c, false, lsm_dt, g.its, g.ite, g.jts, g.jte)) return 1;                         // :1210-1278
    {
        PostArgs a;
        a.d = c->d; a.i0 = g.its - c->ims; a.i1 = g.ite - c->ims; a.j0 = g.jts - c->jms; a.j1 = g.jte - c->jms;
        a.max_swe = icar_noah_max_swe(c);
        a.z_atm = s->arr[ICAR_LSM_Z_ATM]; a.znt = (const float *)c->field[ICAR_F_ROUGHNESS_Z0]; a.emiss = icar_noah_array(c, ICAR_NOAH_EMISS);
        a.tskin = (const float *)c->field[ICAR_F_SKIN_TEMPERATURE]; a.smois = icar_noah_array(c, ICAR_NOAH_SOIL_WATER_CONTENT);
        a.hfx = (const float *)c->field[ICAR_F_SENSIBLE_HEAT]; a.qfx = (const float *)c->field[ICAR_F_QFX]; a.qsfc = (const float *)c->field[ICAR_F_QSFC];
        a.chs2 = icar_noah_array(c, ICAR_NOAH_CHS2); a.cqs2 = icar_noah_array(c, ICAR_NOAH_CQS2); a.psfc = (const float *)c->field[ICAR_F_SURFACE_PRESSURE];
        a.precip = (const double *)c->field[ICAR_F_PRECIPITATION];
        a.swe = icar_noah_array(c, ICAR_NOAH_SNOW_WATER_EQUIVALENT); a.lnz = s->arr[ICAR_LSM_LNZ_ATM_TERM]; a.base = s->arr[ICAR_LSM_BASE_EXCHANGE_TERM];
        a.lwup = s->arr[ICAR_LSM_LONGWAVE_UP]; a.smstot = icar_noah_array(c, ICAR_NOAH_SOIL_TOTALMOISTURE); a.t2 = s->arr[ICAR_LSM_TEMPERATURE_2M];
        a.q2 = s->arr[ICAR_LSM_HUMIDITY_2M]; a.rainbl = s->rainbl;
        if (!a.qfx || !a.qsfc) { icar_set_error("lsm: QFX / QSFC are not on the device"); return 1; }  // (icar_noah_run has made them)
        ScopedTimer timer(c, "lsm_noah_post");
        hipLaunchKernelGGL(k_lsm_noah_post, grid, block, 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

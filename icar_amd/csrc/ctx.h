// icar_amd/csrc/ctx.h -- device context behind the C ABI (include/icar_hip.h).
// Replaces the reference's module-level SAVE state (adv_upwind/adv_mpdata U_m,V_m,W_m;
// microphysics SR,last_model_time; Thompson tables) with one handle per image/GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <map>
#include <vector>
#include "../../include/icar_hip.h"

#define ICAR_MAX_ADV 12

struct Dims {
    int nx, nz, ny;      // memory extents (ime-ims+1, ...)
    int sk, sj;          // strides of k and j (sk = nx, sj = nx*nz)
    __host__ __device__ inline int idx(int i, int k, int j) const { return i + nx * (k + nz * j); }
};

struct VarPtrs { float *p[ICAR_MAX_ADV]; };
struct CVarPtrs { const float *p[ICAR_MAX_ADV]; };

struct TimingGroup { double total_ms = 0; int launches = 0; };

struct ThompsonTables;   // mp_thompson.hip
struct LinWinds;         // linear_winds.hip
struct Wsm3State;        // mp_wsm3.hip
struct Wsm6State;        // mp_wsm6.hip
struct IcarComm;         // comm.hip
struct CuState;          // cu_bmj.hip
struct YsuState;         // pbl_ysu.hip
struct ForcingState;     // forcing.hip
struct Forcing2dState;   // forcing2d.hip
struct NoahState;        // lsm_noah.hip
struct LsmDriverState;   // lsm_noah_driver.hip

// state of the step driver (timestep.hip): the options / grid members the sub-step loop reads, the model clock, and what
// mp_driver.f90 keeps in SAVE variables (last_model_time)

struct IcarStepState {
    bool configured = false;
    icar_hip_step_config cfg;
    std::vector<float> dz_levels;
    double model_time = 0.0;                 // domain%model_time%seconds()
    double mp_last_model_time = -999.0;      // mp_driver.f90:44 last_model_time
    int winds_scheme = 0, winds_dens = 0; float winds_dt = 0.f;   // what the Courant winds on the device were set up for
    float *h_val = nullptr;                  // pinned: the reduced CFL maximum
    bool early_open = false, early_wreal = false, early_face = false;   // a sub-step whose dt-independent opening is already in flight
    bool early_lazy = false;                 // ... and that opening wrote only the diagnostics the device reads (not a call's last sub-step)
    bool failed = false;                 // a sub-step was abandoned half-applied (timestep.hip: update_dt_opened): the fields are not a model state any more
    bool winds_first = true;                 // wind.f90:297 `.not. allocated(domain%sintheta)`: update_winds has not run yet
    int boundarylayer = 0;                   // options%physics%boundarylayer (icar_hip_pbl_configure / _pbl_init): 0, 1, ICAR_PBL_SIMPLE or ICAR_PBL_YSU
    int radiation = 0;                       // options%physics%radiation (icar_hip_rad_configure): 0, 1 or ICAR_RA_SIMPLE
    // icar_hip_rad_calendar: the calendar and, on the library's clock, 1 January 00:00 of the model time's year with the lengths of that year and the next
    bool rad_calendar_set = false;
    int rad_calendar = 0;
    double rad_year_start = 0.0, rad_year_days = 365.0, rad_next_year_days = 365.0;
    // icar_hip_lsm_configure: options%physics%landsurface / %watersurface, options%lsm_options, lsm_driver.f90's SAVE variable last_model_time
    int landsurface = 0, watersurface = 0, lsm_update_interval = 300;
    float sh_feedback_fraction = 0.625f, lh_feedback_fraction = 1.0f, sfc_layer_thickness = 400.0f;
    double lsm_last_model_time = -999.0;
    // icar_hip_cu_configure: options%physics%convection (0, ICAR_CU_BMJ, ICAR_CU_TIEDTKE or ICAR_CU_NSAS) and options%cu_options with the fractions already inherited
    int convection = 0;
    float cu_tendency_fraction = 1.0f, cu_tend_qv_fraction = 1.0f, cu_tend_qc_fraction = 1.0f, cu_tend_th_fraction = 1.0f, cu_tend_qi_fraction = 1.0f;
};

// component indices of the per-cell coefficients in icar_hip_ctx::mpc (k_mpdata_coef in mpdata.hip says what they hold): the first
// nine are the antidiffusive coefficients of the x / y / z faces, the last two the denominators jaco rho and dz jaco rho of the
// donor-cell passes.  They are stored as tuples, not as arrays: floats [3 n3 f, 3 n3 (f+1)) hold face f's (x, y, z) tuple
// {MPC_A?, MPC_C??, MPC_C??} of every cell (12 B stride), so the first MPC_GH n3 floats are exactly the nine antidiffusive
// coefficients; behind them, from mpc_cell_bytes(n3) on, one 16-B tuple {GH, GV, U_m, W_m} per cell (copies of icar_hip_ctx::U, W).
enum { MPC_AU = 0, MPC_CUV, MPC_CUW, MPC_AV, MPC_CVU, MPC_CVW, MPC_AW, MPC_CWU, MPC_CWV, MPC_GH, MPC_GV, MPC_N };
__host__ __device__ inline size_t mpc_cell_bytes(size_t n3) { return (MPC_GH * n3 * sizeof(float) + 255) & ~(size_t)255; }
__host__ __device__ inline size_t mpc_bytes(size_t n3) { return mpc_cell_bytes(n3) + 4 * n3 * sizeof(float); }

struct icar_hip_ctx {
    int device = 0;
    int ims, ime, kms, kme, jms, jme;
    Dims d;
    size_t n3 = 0;                       // nx*nz*ny
    hipStream_t stream = nullptr;        // the stream every entry point launches on (main, or aux between aux_begin/aux_end)
    bool own_stream = false;
    // second HIP stream (north_star: halo strips + exchange on one stream, interior work beside them on the other)
    hipStream_t aux = nullptr, main_saved = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool on_aux = false;
    void *field[ICAR_N_FIELD_SLOTS] = {nullptr};
    float *dqdt[ICAR_N_FIELD_SLOTS] = {nullptr};    // variable_t%dqdt_3d mirrors (apply_forcing)
    // advection scratch (A1-A5)
    float *U = nullptr, *V = nullptr, *W = nullptr, *Wdz = nullptr;
    float *mpc = nullptr;                // MPDATA: the scalar-independent coefficients of this step's winds, mpc_bytes(n3) (MPC_* above)
    int mpc_dens = -1;
    float *alt[ICAR_N_ADVECTABLE] = {nullptr};   // ping-pong partner of each advected scalar
    float *mpx_buf = nullptr;            // mpdata_exact.hip: q2 (x2), u2, v2, w2 of mpx_nv scalars and the limited velocities of one
    int mpx_nv = 0;
    int mpdata_exact = 0;                // icar_hip_mpdata_exact: corrective iterations in the reference's operation order (bit-exact)
    bool winds_valid = false;
    // u / v / w bookkeeping for the prefetched CFL reduction (icar_hip_max_courant_prefetch): every entry point that writes a wind
    // field bumps the version; a raw device pointer to one of them handed out (icar_hip_field_device_ptr) disables the cache
    unsigned long long wind_version = 0;
    bool wind_ptr_escaped = false;
    struct { bool valid = false, reduced = false; unsigned long long ver = 0; float dx = 0.f; std::vector<float> dzl; } cfl_pre;
    float *h_cfl_pre = nullptr;          // pinned host copy of the prefetched maximum (d_red[8] on the device)
    bool cfl_wait_failed = false;        // the wait for that copy failed (compute_dt reports it; a NaN maximum otherwise means NaN winds)
    hipEvent_t cfl_ev = nullptr;
    float *iw_adj = nullptr;             // iterative_winds ADJ scratch (iterative_winds.hip)
    float *wgr_tmp = nullptr;            // make_winds_grid_relative: rotated mass-grid u | v (2 x n3)
    float *pbl_kq = nullptr;             // pbl_simple.hip: Kq_m of the last call (n3), allocated on first use
    unsigned *pbl_rowmax = nullptr;      // pbl_simple.hip: bit pattern of maxval(Kq/dz) of every row (ny)
    float *ra_coslat = nullptr;          // ra_simple.hip: cos_lat_m | sin_lat_m of ra_simple_init (2 x nx*ny), allocated on first use
    bool ra_lat_valid = false;           // ... and whether they are those of the ICAR_F_LATITUDE on the device
    // sfc_basic.hip: apply_fluxes' nz (its SAVE variable) for (kts, kte, sfc_layer_thickness), and the levels' maxima it is found from
    bool sfc_nz_valid = false;
    int sfc_nz = 0, sfc_nz_kts = 0, sfc_nz_kte = 0;
    float sfc_nz_thick = 0.0f;
    unsigned *sfc_levelmax = nullptr;
    CuState *cu = nullptr;               // cu_bmj.hip: the convection slot's arrays, BMJINIT's tables and the column workspace
    NoahState *noah = nullptr;           // lsm_noah.hip: the Noah tables and the model's own arrays (ICAR_NOAH_*)
    LsmDriverState *lsmdrv = nullptr;    // lsm_noah_driver.hip: the ICAR_LSM_* arrays and whether icar_hip_lsm_noah_couple has run since lsm_init
    YsuState *ysu = nullptr;             // pbl_ysu.hip: pbl_init's arrays, the scheme's results and tendencies, the column workspace
    // reductions / flags
    float *d_red = nullptr;              // small device scratch for reductions
    std::vector<float> dzl_host;         // dz_levels last uploaded behind d_red (compute_dt re-sends them only when they change)
    int *d_flag = nullptr;
    ThompsonTables *thompson = nullptr;
    LinWinds *linwinds = nullptr;
    Wsm3State *wsm3 = nullptr;
    Wsm6State *wsm6 = nullptr;
    IcarComm *comm = nullptr;            // halo transport + co_min (comm.hip)
    ForcingState *forcing = nullptr;     // forcing.hip: the look-up tables, the forcing's own arrays, the temporaries of interpolate_forcing
    Forcing2dState *forcing2d = nullptr; // forcing2d.hip: the forced 2-D variables' forcing arrays, dqdt_2d, external_precipitation, the enabled set
    IcarStepState step;                  // timestep.hip
    // timing
    bool timing = false;
    std::string timing_only;             // ",group,group," or empty = every group (icar_hip_timing_groups)
    std::vector<hipEvent_t> event_pool;  // timing events are reused, not created per scope
    std::map<std::string, TimingGroup> timers;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> pending;
};

void icar_set_error(const std::string &msg);
int icar_hip_check(hipError_t e, const char *what);
#define HIPCHK(x) do { if (icar_hip_check((x), #x)) return 1; } while (0)

// field geometry
size_t icar_field_count(const icar_hip_ctx *c, int field);
float *icar_field_f(icar_hip_ctx *c, int field, bool required = true);   // allocates lazily
// the registry's classes of field ids, one definition for every file that asks
inline bool icar_field_is_2dd(int f) { return f == ICAR_F_PRECIPITATION || f == ICAR_F_SNOWFALL || f == ICAR_F_GRAUPEL_ACC || f == ICAR_F_SINTHETA || f == ICAR_F_COSTHETA; }
// a field the Courant winds are made of: rewriting it makes them, and a prefetched CFL maximum, stale (icar_winds_changed)
inline bool icar_field_feeds_winds(int f) { return f == ICAR_F_U || f == ICAR_F_V || f == ICAR_F_W || (f >= ICAR_F_DENSITY && f <= ICAR_F_ADVECTION_DZ); }
// a REAL(4) field with levels: (nx, nz, ny), u's (nx+1, nz, ny) or v's (nx, nz, ny+1) -- what a dqdt_3d mirror can belong to
inline bool icar_field_is_3d(const icar_hip_ctx *c, int f) { return f >= 0 && f < ICAR_N_FIELD_SLOTS && !icar_field_is_2dd(f) && icar_field_count(c, f) >= c->n3; }

// timing helpers
struct ScopedTimer {
    icar_hip_ctx *c; const char *group; hipEvent_t e0 = nullptr, e1 = nullptr;
    ScopedTimer(icar_hip_ctx *c_, const char *g);
    ~ScopedTimer();
};

// capi.hip: what every entry point that reaches the device does first: refuse a null context / pointer, select the context's device
int icar_enter(icar_hip_ctx *c, const char *who, bool pointers_ok = true);
inline void icar_winds_changed(icar_hip_ctx *c) { c->winds_valid = false; ++c->wind_version; }   // u, v, w (or density / jacobians) rewritten

// the rows, under the file that defines them
// advect.hip
int icar_advect_setup_winds(icar_hip_ctx *c, int scheme, float dt, float dx, int advect_density, bool with_wreal = false, bool *wreal_done = nullptr);
int icar_advect_run(icar_hip_ctx *c, int scheme, int order, int fct, int advect_density, const int *fields, int n);
// mp_simple.hip
int icar_mp_simple_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte, int *err);
int icar_mp_simple_run_tiles(icar_hip_ctx *c, float dt, int ntiles, const int tiles[][4], int kts, int kte, int *err);
// pbl_simple.hip
int icar_pbl_simple_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_pbl_run(icar_hip_ctx *c, float dt);                                // pbl(domain, options, dt): the configured scheme on the step's tile
int icar_pbl_nsubsteps_copy(icar_hip_ctx *c, int *out, int n);
inline bool icar_pbl_on(const icar_hip_ctx *c) { return c->step.boundarylayer == ICAR_PBL_SIMPLE || c->step.boundarylayer == ICAR_PBL_YSU; }   // pbl() does something
// pbl_ysu.hip
void icar_ysu_free(icar_hip_ctx *c);
int icar_ysu_init_device(icar_hip_ctx *c);                                  // pbl_init for kPBL_YSU: arrays, z_atm, gz1oz0, zol, hol, workspace
int icar_ysu_sfc_run(icar_hip_ctx *c, float dx);                            // pbl_driver.f90:227-254
int icar_ysu_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);   // the call of ysu alone (kte the model's)
int icar_ysu_pbl_run(icar_hip_ctx *c, float dt);                            // pbl(domain, options, dt) for kPBL_YSU on the step's tile
int icar_ysu_copy(icar_hip_ctx *c, int which, void *host, size_t n, bool to_device);
const float *icar_ysu_hpbl(const icar_hip_ctx *c);                         // ICAR_YSU_HPBL on the device, or null while YSU is not initialised
// ra_simple.hip
int icar_ra_simple_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte, int runlw, int calendar, double D, double year_days);
int icar_rad_clock(icar_hip_ctx *c, double model_time, double *D, double *year_days);   // day of the year under icar_hip_rad_calendar's anchor
int icar_rad_run(icar_hip_ctx *c, float dt);                                // rad(domain, options, dt): the configured scheme on the step's tile
// sfc_basic.hip
int icar_sfc_diag_10m_run(icar_hip_ctx *c);                                 // time_step.f90:143-161
int icar_sfc_water_simple_run(icar_hip_ctx *c);
int icar_sfc_layers(icar_hip_ctx *c, int kts, int kte, int *nz_out);
int icar_sfc_apply_fluxes_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_lsm_run(icar_hip_ctx *c, float dt);                                // lsm(domain, options, dt): the gate, water_simple, apply_fluxes on the step's tile
int icar_lsm_init_device(icar_hip_ctx *c);
// lsm_noah.hip
void icar_noah_free(icar_hip_ctx *c);
bool icar_noah_ready(const icar_hip_ctx *c);                                // tables on the device and icar_hip_lsm_init run since the last tables / categories
float *icar_noah_array(icar_hip_ctx *c, int which);                         // an ICAR_NOAH_* array (icar_noah_ready)
float icar_noah_max_swe(const icar_hip_ctx *c);
int icar_noah_run(icar_hip_ctx *c, bool chs_from_host, float lsm_dt, int its, int ite, int jts, int jte);   // the call of lsm_noah
// lsm_noah_driver.hip
void icar_lsm_driver_free(icar_hip_ctx *c);
void icar_lsm_uncouple(icar_hip_ctx *c);                                    // a new lsm_init / lsm_configure: lsm() refuses Noah again
bool icar_lsm_noah_coupled(const icar_hip_ctx *c);                          // icar_hip_lsm_noah_couple has run and Noah is still initialised
int icar_lsm_noah_gated_run(icar_hip_ctx *c, float lsm_dt);                 // the gated block of lsm() for kLSM_NOAH (lsm_driver.f90:1028-1546)
// cu_bmj.hip
void icar_cu_free(icar_hip_ctx *c);
int icar_cu_init_device(icar_hip_ctx *c);                                   // init_convection for kCU_BMJ: arrays, tables, workspace
int icar_cu_bmj_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_convect_run(icar_hip_ctx *c, float dt);                            // convect(domain, options, dt) on the step's tile
int icar_cu_copy(icar_hip_ctx *c, int which, void *host, bool to_device);
int icar_cu_reset_run(icar_hip_ctx *c);
int icar_cu_tables_copy(icar_hip_ctx *c, float *out, size_t capacity, size_t *n_out);
// cu_tiedtke.hip
int icar_tiedtke_init_device(icar_hip_ctx *c, const float *znu);           // init_convection for kCU_TIEDTKE: arrays, znu, workspace
int icar_tiedtke_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);   // CU_TIEDTKE alone (kte the model's)
int icar_tiedtke_copy(icar_hip_ctx *c, int which, void *host, bool to_device);
// cu_nsas.hip
int icar_nsas_init_device(icar_hip_ctx *c, float dx);                      // init_convection for kCU_NSAS: arrays, hpbl, workspace
int icar_nsas_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);   // cu_nsas alone (kte the model's)
int icar_nsas_copy(icar_hip_ctx *c, int which, void *host, bool to_device);
// timestep.hip
int icar_mp_run(icar_hip_ctx *c, double dt_in, int halo, int subset, bool exner_from_p = false);   // halo / subset < 0: argument not present
int icar_update_dt(icar_hip_ctx *c, double *seconds);
int icar_substep(icar_hip_ctx *c, double dt, bool enforce, bool last = true);
// halo_pack.hip
int icar_halo_pack_dirs(icar_hip_ctx *c, int ndir, const int *dirs, int halo, const int *fields, int n, void *const *bufs, bool unpack);
int icar_box_copy(icar_hip_ctx *c, int field, int which, int i0, int ni, int j0, int nj, float *buf, bool unpack);
// cfl.hip
int icar_max_courant_run(icar_hip_ctx *c, float dx, const float *dz_levels, float *out, float *d_out);
int icar_max_abs_winds_run(icar_hip_ctx *c, float *out3);
int icar_max_courant_prefetch_run(icar_hip_ctx *c, float dx, const float *dz_levels, bool allreduce);
bool icar_cfl_prefetched_global(icar_hip_ctx *c, float dx, const float *dz_levels, float *value);
bool icar_cfl_prefetch_waiting(icar_hip_ctx *c);      // a prefetched CFL maximum of the current winds is waiting for update_dt
// iterative_winds.hip
int icar_balance_uvw_run(icar_hip_ctx *c, float dx, int update);
int icar_iterative_winds_correct_w(icar_hip_ctx *c, int update);
int icar_mass_conservative_acceleration(icar_hip_ctx *c, int update);
int icar_iterative_winds_sweep(icar_hip_ctx *c, float dx, int nsweeps, int update);
int icar_make_winds_grid_relative(icar_hip_ctx *c, int update);
// step.hip
enum { ICAR_DIAG_CELL = 4, ICAR_DIAG_FACE = 8, ICAR_DIAG_EXNER_RHO = 32 };     // finer parts of icar_diagnostic_update_run, internal
enum { ICAR_LAZY_EXNER_IN_THOMPSON = -1 };     // timestep.hip (lazy_diag_part): no diagnostic launch, Thompson computes exner from the pressure
int icar_diagnostic_update_run(icar_hip_ctx *c, int parts);
bool icar_diag_columns_on(const icar_hip_ctx *c);      // column integrals (ivt, iwv, iwl, iwi) are computed on the device
int icar_apply_forcing_run(icar_hip_ctx *c, double dt, const int *fields, const int *fb, int n, int w, int e, int s, int nn);
int icar_enforce_limits_run(icar_hip_ctx *c, const int *fields, int n);
// mp_thompson.hip, thompson_tables.hip
int icar_thompson_init_run(icar_hip_ctx *c, const float *params, const int *flags);
int icar_thompson_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte,
                      int ids, int ide, int jds, int jde, int kds, int kde, bool exner_from_p = false);
int icar_thompson_run_tiles(icar_hip_ctx *c, float dt, int ntiles, const int (*tiles)[4], int kts, int kte,
                            int ids, int ide, int jds, int jde, int kds, int kde, bool exner_from_p = false);
int icar_thompson_prepare_constants(icar_hip_ctx *c);
void icar_thompson_free(icar_hip_ctx *c);
int icar_thompson_table_download(icar_hip_ctx *c, const char *name, double *out, size_t cap, size_t *n_out);
// mp_wsm3.hip, mp_wsm6.hip
void icar_wsm3_free(icar_hip_ctx *c);
int icar_wsm3_init_run(icar_hip_ctx *c);
int icar_wsm3_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);
void icar_wsm6_free(icar_hip_ctx *c);
int icar_wsm6_init_run(icar_hip_ctx *c);
int icar_wsm6_run(icar_hip_ctx *c, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_wsm6_run_tiles(icar_hip_ctx *c, float dt, int ntiles, const int tiles[][4], int kts, int kte);
// linear_winds.hip
void icar_linwinds_free(icar_hip_ctx *c);
int icar_linwinds_setup_run(icar_hip_ctx *c, const icar_hip_lt_options *o, const float *terrain, int nxg, int nyg, int ids, int jds, float dx);
int icar_linear_perturbation_run(icar_hip_ctx *c, float U, float V, float Nsq, float zb, float zt, float minimum_step, double *u_out, double *v_out);
int icar_linwinds_build_lut_run(icar_hip_ctx *c, const float *zb, const float *zt, int nlev);
int icar_linwinds_build_lut_varying_run(icar_hip_ctx *c, const float *zb3, const float *zt3, int nlev);
int icar_linwinds_lut_copy(icar_hip_ctx *c, int comp, float *host, int to_dev);
int icar_linwinds_lut_entry(icar_hip_ctx *c, int comp, int k, int i, int j, float *host);
int icar_linwinds_pert_copy(icar_hip_ctx *c, int comp, float *host, int to_dev);
int icar_linwinds_terrain_frequency(icar_hip_ctx *c, double *out, size_t cap, int *fnx, int *fny);
int icar_spatial_winds_run(icar_hip_ctx *c, int update);
// ... its smooth_array_3d (ydim = 3) pair, which forcing.hip launches on the forcing's u / v too: in (nx, nz, ny) -> row means -> out
__global__ void k_lw_rowmeans(Dims d, int w, const float *__restrict__ in, double *__restrict__ rowmeans);
__global__ void k_lw_colsmooth(Dims d, int w, const double *__restrict__ rowmeans, float *__restrict__ out);
// forcing.hip
void icar_forcing_free(icar_hip_ctx *c);
int icar_interpolate_forcing_run(icar_hip_ctx *c, const int *fields, int n, int pressure_field, int theta_field, int update);
int icar_update_delta_fields_run(icar_hip_ctx *c, const int *fields, int n, double dt);
// ... the mass grid's geolut as forcing_configure stored it (false: not configured), for forcing2d.hip
struct IcarGeo2d { const int4 *x, *y; const float4 *w; int nx, ny, nx_f, ny_f; };
bool icar_forcing_mass_geo(const icar_hip_ctx *c, IcarGeo2d *g);
// forcing2d.hip
void icar_forcing2d_free(icar_hip_ctx *c);
int icar_forcing2d_apply_run(icar_hip_ctx *c, double dt);                   // apply_forcing's 2-D statements for the enabled set (nothing enabled: no launch)
int icar_forcing2d_step_check(icar_hip_ctx *c, const char *who, double dt); // forcing_step: what the enabled set would be refused for
int icar_forcing2d_step_run(icar_hip_ctx *c, double dt);                    // forcing_step: geo_interp2d (update) and the 2-D delta of the enabled set

/* include/icar_hip.h -- C ABI of libicar_hip.so: the MI355X (gfx950) implementation of ICAR's
 * per-timestep 3-D grid update (advection + column microphysics + wind balance + halo faces).
 *
 * Every entry point replaces one Fortran procedure of the reference (NCAR/icar, cited as
 * src/...:line).  The reference has no C ABI of its own; the seam chosen is its level-2 physics
 * kernels, which already take plain REAL(4) arrays + WRF-style index triplets.
 * The Fortran-2008 iso_c_binding module that binds these (icar_amd/fortran/icar_hip_mod.f90)
 * and the call sites a maintainer edits are shown in INTEGRATION.md.
 *
 * Conventions
 *  - All 3-D fields are REAL(4) in Fortran order X(ims:ime, kms:kme, jms:jme): i (x) fastest,
 *    then k (z), then j (y).  u is staggered (ims:ime+1), v is (jms:jme+1).
 *    2-D accumulators are REAL(8) X(ims:ime, jms:jme) like domain%...%data_2dd.
 *  - Index arguments (its..kte, ids..kde) are in the same index space as the ims..jme given at
 *    context creation (any lower bound), inclusive, exactly as the reference passes them.
 *  - Functions return 0 on success, non-zero on error; icar_hip_last_error() gives the text.
 *    (The reference's convention is `stop`/`error stop`; the Fortran binding maps !=0 to error stop.)
 *  - One context per coarray image / GPU; calls on a context are serialised by the caller
 *    (same as the reference's module-level SAVE state, which the context replaces).
 *  - No CPU fallback exists: without a visible gfx950 device icar_hip_ctx_create fails.
 */
#ifndef ICAR_HIP_H
#define ICAR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct icar_hip_ctx icar_hip_ctx;

/* Field ids mirror the domain_t members the path touches (src/objects/domain_h.f90:35-50,283-293)
 * and the kVARS order used by the advection dispatch (src/physics/adv_mpdata.f90:512-522). */
enum icar_hip_field {
    ICAR_F_WATER_VAPOR = 0,        /* domain%water_vapor%data_3d            */
    ICAR_F_CLOUD_WATER = 1,        /* domain%cloud_water_mass%data_3d       */
    ICAR_F_RAIN = 2,               /* domain%rain_mass%data_3d              */
    ICAR_F_SNOW = 3,               /* domain%snow_mass%data_3d              */
    ICAR_F_POTENTIAL_TEMPERATURE = 4,
    ICAR_F_CLOUD_ICE = 5,          /* domain%cloud_ice_mass%data_3d         */
    ICAR_F_GRAUPEL = 6,            /* domain%graupel_mass%data_3d           */
    ICAR_F_ICE_NUMBER = 7,         /* domain%cloud_ice_number%data_3d       */
    ICAR_F_RAIN_NUMBER = 8,        /* domain%rain_number%data_3d            */
    ICAR_F_SNOW_NUMBER = 9,        /* domain%snow_number%data_3d            */
    ICAR_F_GRAUPEL_NUMBER = 10,    /* domain%graupel_number%data_3d         */
    ICAR_N_ADVECTABLE = 11,
    ICAR_F_U = 11,                 /* domain%u%data_3d   (nx+1, nz, ny)     */
    ICAR_F_V = 12,                 /* domain%v%data_3d   (nx, nz, ny+1)     */
    ICAR_F_W = 13,                 /* domain%w%data_3d                      */
    ICAR_F_PRESSURE = 14,
    ICAR_F_EXNER = 15,
    ICAR_F_DENSITY = 16,
    ICAR_F_DZ_MASS = 17,           /* domain%dz_mass%data_3d                */
    ICAR_F_JACOBIAN = 18,          /* domain%jacobian                       */
    ICAR_F_JACOBIAN_U = 19,        /* (nx+1, nz, ny)                        */
    ICAR_F_JACOBIAN_V = 20,        /* (nx, nz, ny+1)                        */
    ICAR_F_JACOBIAN_W = 21,
    ICAR_F_ADVECTION_DZ = 22,      /* domain%advection_dz                   */
    ICAR_F_PRECIPITATION = 23,     /* domain%accumulated_precipitation%data_2dd  REAL(8) (nx,ny) */
    ICAR_F_SNOWFALL = 24,          /* domain%accumulated_snowfall%data_2dd       REAL(8) (nx,ny) */
    ICAR_F_GRAUPEL_ACC = 25,       /* domain%graupel%data_2dd                    REAL(8) (nx,ny) */
    /* diagnostic_update outputs / inputs (src/main/time_step.f90:49-198) */
    ICAR_F_PRESSURE_INTERFACE = 26,
    ICAR_F_TEMPERATURE = 27,
    ICAR_F_TEMPERATURE_INTERFACE = 28,
    ICAR_F_U_MASS = 29,
    ICAR_F_V_MASS = 30,
    ICAR_F_W_REAL = 31,
    ICAR_F_DZDX = 32,              /* domain%dzdx  (nx+1, nz, ny)           */
    ICAR_F_DZDY = 33,              /* domain%dzdy  (nx, nz, ny+1)           */
    ICAR_F_SURFACE_PRESSURE = 34,  /* domain%surface_pressure%data_2d  REAL(4) (nx,ny) */
    /* linear-theory winds (src/physics/linear_winds.f90:840-1127) */
    ICAR_F_Z = 35,                 /* domain%z%data_3d (mass-level height)  */
    ICAR_F_NSQUARED = 36,          /* domain%nsquared%data_3d               */
    /* optional column integrals of diagnostic_update (src/main/time_step.f90:126-144), REAL(4) (nx,ny) */
    ICAR_F_IVT = 37,               /* domain%ivt%data_2d  integrated vapour transport            */
    ICAR_F_IWV = 38,               /* domain%iwv%data_2d  integrated water vapour                */
    ICAR_F_IWL = 39,               /* domain%iwl%data_2d  integrated liquid (cloud + rain)       */
    ICAR_F_IWI = 40,               /* domain%iwi%data_2d  integrated ice (ice + snow + graupel)  */
    /* update_winds, windtype kCONSERVE_MASS (src/physics/wind.f90:301-306): the host uploads domain%zr_u / zr_v, or
     * zfr_u / zfr_v when options%parameters%use_terrain_difference */
    ICAR_F_ZR_U = 41,              /* (nx+1, nz, ny)                        */
    ICAR_F_ZR_V = 42,              /* (nx, nz, ny+1)                        */
    /* make_winds_grid_relative (src/physics/wind.f90:236-287): domain%sintheta / costheta, REAL(8) (nx,ny) */
    ICAR_F_SINTHETA = 43,
    ICAR_F_COSTHETA = 44,
    /* simple_pbl (src/physics/pbl_simple.f90:69-86): read-only surface description, uploaded once */
    ICAR_F_TERRAIN = 45,           /* domain%terrain%data_2d  REAL(4) (nx,ny)    */
    ICAR_F_LAND_MASK = 46,         /* domain%land_mask  INTEGER(4) (nx,ny): kLC_LAND = 1, kLC_WATER = 2 */
    ICAR_N_FIELDS = 47,            /* the ids 0 .. 46 above; kept at this value for hosts that size tables of their own by it */
    /* ra_simple (src/physics/ra_simple.f90:191-272), a block of its own behind the fields above: inputs in degrees as
     * domain%latitude%data_2d / %longitude%data_2d hold them, uploaded once; outputs domain%shortwave / %longwave /
     * %cloud_fraction (data_2d).  REAL(4) (nx,ny) */
    ICAR_F_LATITUDE = 47,
    ICAR_F_LONGITUDE = 48,
    ICAR_F_SHORTWAVE = 49,
    ICAR_F_LONGWAVE = 50,
    ICAR_F_CLOUD_FRACTION = 51,
    ICAR_N_FIELD_IDS = 52,         /* the ids 0 .. 51 above (the fields and ra_simple's block); kept at this value like ICAR_N_FIELDS */
    /* the surface-flux slot (src/physics/lsm_driver.f90 with landsurface = kLSM_BASIC, src/physics/water_simple.f90) and the 10 m
     * diagnostics of diagnostic_update (src/main/time_step.f90:143-161), a block of its own.  REAL(4) (nx,ny) unless said otherwise */
    ICAR_F_ROUGHNESS_Z0 = 52,      /* domain%roughness_z0%data_2d: uploaded = `associated`; rewritten over open water by water_simple */
    ICAR_F_U_10M = 53,             /* domain%u_10m%data_2d   (0 outside ims+1:ime-1, jms+1:jme-1)       */
    ICAR_F_V_10M = 54,             /* domain%v_10m%data_2d                                               */
    ICAR_F_USTAR = 55,             /* domain%ustar           (0.1 outside that range, domain_obj.f90:419) */
    ICAR_F_SST = 56,               /* domain%sst%data_2d                                                 */
    ICAR_F_SKIN_TEMPERATURE = 57,  /* domain%skin_temperature%data_2d                                    */
    ICAR_F_SENSIBLE_HEAT = 58,     /* domain%sensible_heat%data_2d                                       */
    ICAR_F_LATENT_HEAT = 59,       /* domain%latent_heat%data_2d                                         */
    ICAR_F_QSFC = 60,              /* lsm_driver.f90's module-private QSFC, readable for tests           */
    ICAR_F_QFX = 61,               /* lsm_driver.f90's module-private QFX, readable for tests            */
    ICAR_F_DZ_INTERFACE = 62,      /* domain%dz_interface%data_3d  (nx, nz, ny)                          */
    ICAR_N_FIELD_SLOTS = 63        /* every id an entry point takes is below this one; sizes the library's tables */
};

enum { ICAR_ADV_UPWIND = 1, ICAR_ADV_MPDATA = 2 };   /* kADV_UPWIND / kADV_MPDATA, icar_constants.f90:341 */

/* ---- context + device-resident field mirrors (replaces module SAVE state) ---- */
int icar_hip_ctx_create(icar_hip_ctx **ctx, int device,
                        int ims, int ime, int kms, int kme, int jms, int jme);
int icar_hip_ctx_destroy(icar_hip_ctx *ctx);
/* Run all kernels of this context on the caller's HIP stream (hipStream_t); NULL = own stream. */
int icar_hip_set_stream(icar_hip_ctx *ctx, void *hip_stream);
int icar_hip_synchronize(icar_hip_ctx *ctx);
/* Second HIP stream of the context (created on first use).  time_step.f90:512-526 orders
 *     mp(halo=1) -> halo_send -> mp(subset=1) -> halo_retrieve
 * so that the interior microphysics overlaps the coarray PUTs; here the strips, the pack kernels and the exchange stay
 * on the main stream while the interior launch runs beside them on the aux stream:
 *     aux_fork   aux waits for everything issued on the main stream so far
 *     aux_begin  ... entry points called here launch on the aux stream ...  aux_end
 *     aux_join   the main stream waits for everything issued on the aux stream so far
 * Work issued between fork and join on the two streams must touch disjoint cells (strips vs interior columns). */
int icar_hip_aux_fork(icar_hip_ctx *ctx);
int icar_hip_aux_begin(icar_hip_ctx *ctx);
int icar_hip_aux_end(icar_hip_ctx *ctx);
int icar_hip_aux_join(icar_hip_ctx *ctx);
/* Lazily allocates the device mirror of a field.  Host buffers are the domain_t arrays
 * (contiguous, Fortran order).  Element count: icar_hip_field_count(). */
int icar_hip_field_upload(icar_hip_ctx *ctx, int field, const void *host);
int icar_hip_field_download(icar_hip_ctx *ctx, int field, void *host);
int icar_hip_field_fill(icar_hip_ctx *ctx, int field, double value);
/* Current device pointer of a field (advect() ping-pongs the advected scalars, so re-query
 * after every icar_hip_advect call). */
int icar_hip_field_device_ptr(icar_hip_ctx *ctx, int field, void **dptr);
size_t icar_hip_field_count(const icar_hip_ctx *ctx, int field);
size_t icar_hip_field_elem_size(int field);

/* ---- A1: Courant-number winds U_m,V_m,W_m -----------------------------------------------------
 * replaces setup_module_winds (src/physics/advect.f90:306-351, scheme=1) and the inline block of
 * mpdata (src/physics/adv_mpdata.f90:496-506, scheme=2; the two differ in multiplication order). */
int icar_hip_setup_winds(icar_hip_ctx *ctx, int scheme, float dt, float dx, int advect_density);

/* ---- A2-A5: advect the listed scalars with the winds of the last icar_hip_setup_winds --------
 * replaces the per-variable advect3d dispatch of upwind (src/physics/advect.f90:380-418) and
 * mpdata (src/physics/adv_mpdata.f90:463-524; advect3d :356-418, upwind_advection :44-105,
 * mpdata_fluxes :107-255, flux_limiter :257-354 + adv_mpdata_FCT_core.f90:47-116).
 * fields[] are ICAR_F_* ids < ICAR_N_ADVECTABLE (the caller derives them from
 * options%vars_to_advect); mpdata_order / fct = options%adv_options.
 * Call icar_hip_setup_winds again whenever u, v, w, density or a jacobian changed on the device (apply_forcing,
 * balance_uvw, the wind solvers): the call fails if the Courant winds are known to be stale.
 * Arithmetic: the upwind scheme (and mpdata_order 1) is bit-identical to the reference; MPDATA's corrective iterations
 * use 1-ulp reciprocals and agree with it to 1e-5 of the local field scale (tests/test_gpu_advect.py). */
int icar_hip_advect(icar_hip_ctx *ctx, int scheme, int mpdata_order, int fct, int advect_density,
                    const int *fields, int nfields);

/* Corrective iterations of MPDATA in the reference's own operation order (on = 1): donor cell, mpdata_fluxes, flux_limiter +
 * FCT core and the final donor cell as separate launches per scalar, IEEE division, no contraction -- the advected fields are
 * then BIT-IDENTICAL to src/physics/adv_mpdata.f90:356-418 on the CPU, and so is a whole sub-step sequence
 * (tests/test_gpu_advect.py, tests/test_gpu_trajectory.py).  Costs ~100 B of HBM traffic per scalar-cell instead of 8; the
 * default (on = 0) is the fused kernel.  No counterpart in the reference (it has one arithmetic). */
int icar_hip_mpdata_exact(icar_hip_ctx *ctx, int on);
/* 1 while the Courant winds of the last icar_hip_setup_winds still belong to the state (nothing has rewritten u, v, w, density
 * or a jacobian since), else 0: a host that launches the setup early -- beside the interior microphysics, see INTEGRATION.md --
 * asks before it skips the setup in advect(). */
int icar_hip_winds_valid(icar_hip_ctx *ctx);

/* ---- M1: mp_simple_driver (src/physics/mp_simple.f90:595-646) on the tile its..kte -----------
 * uses PRESSURE, POTENTIAL_TEMPERATURE, EXNER, DENSITY, WATER_VAPOR, CLOUD_WATER, RAIN, SNOW,
 * DZ_MASS; adds the tile's surface fluxes to PRECIPITATION / SNOWFALL exactly as
 * process_subdomain does (src/physics/mp_driver.f90:587-595).  *err_count (may be NULL) receives
 * the number of columns on which the reference would have hit its `stop` in phase_change. */
int icar_hip_mp_simple(icar_hip_ctx *ctx, float dt,
                       int its, int ite, int jts, int jte, int kts, int kte, int *err_count);
/* process_halo's strips (src/physics/mp_driver.f90:609-658: one process_subdomain -> mp_simple_driver call per strip) as
 * ONE launch over up to 4 non-overlapping tiles {its,ite,jts,jte} (as icar_hip_mp_tiles returns them). */
int icar_hip_mp_simple_tiles(icar_hip_ctx *ctx, float dt, int ntiles, const int tiles[][4], int kts, int kte, int *err_count);

/* ---- M2-M4: Thompson microphysics ------------------------------------------------------------
 * thompson_init (src/physics/mp_thompson.f90:342-766; params/flags = mp_options_type in the
 * order Nt_c,TNO,am_s,rho_g,av_s,bv_s,fv_s,av_g,bv_g,av_i,Ef_si,Ef_rs,Ef_rg,Ef_ri,C_cubes,
 * C_sqrd,mu_r,t_adjust ; Ef_rw_l,Ef_sw_l) and mp_gt_driver (:772-1044). */
int icar_hip_thompson_init(icar_hip_ctx *ctx, const float params[18], const int flags[2]);
int icar_hip_thompson(icar_hip_ctx *ctx, float dt,
                      int its, int ite, int jts, int jte, int kts, int kte,
                      int ids, int ide, int jds, int jde, int kds, int kde);

/* process_halo (src/physics/mp_driver.f90:609-658) calls process_subdomain -> mp_gt_driver once per strip; the four
 * one-cell strips are latency-bound when launched one after another, so this entry runs up to 4 tiles
 * {its,ite,jts,jte} (as icar_hip_mp_tiles returns them) in ONE launch.  Tiles must not overlap. */
int icar_hip_thompson_tiles(icar_hip_ctx *ctx, float dt, int ntiles, const int tiles[][4], int kts, int kte,
                            int ids, int ide, int jds, int jde, int kds, int kde);
/* Download one Thompson lookup table by its reference name (tcg_racg ... t_Efsw, Fortran order) for
 * cross-checks against ICAR's own qr_acr_qg_mpt.dat / qr_acr_qs_mpt.dat / freezeH2O_mpt.dat caches
 * (src/physics/mp_thompson.f90:2870-2887).  out may be NULL to query the element count. */
int icar_hip_thompson_table(icar_hip_ctx *ctx, const char *name, double *out, size_t capacity, size_t *count);

/* ---- M0: tile bookkeeping of mp()/process_halo (src/physics/mp_driver.f90:609-772) -----------
 * Fills tiles[n][4] = {its,ite,jts,jte} for halo>0 (W,E,S,N strips; corners once) or for the
 * interior shrunk by subset; returns the number of tiles (integer-exact restatement). */
int icar_hip_mp_tiles(int its, int ite, int jts, int jte, int halo, int subset, int tiles[4][4]);

/* ---- WSM3 (src/physics/mp_wsm3.f90), the kMP_WSM3 slot of mp()'s dispatch (mp_driver.f90:103-106, :552-585) -------------
 * wsm3_init == wsm3init(rhoair0, rhowater, rhosnow, cliq, cpv).  wsm3 == process_subdomain's call: qci = CLOUD_WATER,
 * qrs = RAIN, w = W_REAL, den = DENSITY, pii = EXNER, delz = DZ_MASS; precipitation / snowfall of the call are added to the
 * REAL(8) ICAR_F_PRECIPITATION / ICAR_F_SNOWFALL (:587-595).  Tile bounds 1-based inclusive like its..kte. */
int icar_hip_wsm3_init(icar_hip_ctx *ctx);
int icar_hip_wsm3(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte);

/* ---- WSM6 (src/physics/mp_wsm6.f90), the kMP_WSM6 slot of mp()'s dispatch (mp_driver.f90:98-101, :518-550) ----------------
 * wsm6_init == wsm6init(rhoair0, rhowater, rhosnow, cliq, cpv) (:1432-1506).  wsm6 == process_subdomain's call of wsm6 (:62):
 * q = WATER_VAPOR, qc = CLOUD_WATER, qi = CLOUD_ICE, qr = RAIN, qs = SNOW, qg = GRAUPEL, th = POTENTIAL_TEMPERATURE, with
 * EXNER, PRESSURE, DZ_MASS, DENSITY; the tile's rain / snow / graupel surface sums are added to PRECIPITATION, SNOWFALL and
 * GRAUPEL_ACC as mp_driver.f90:587-595 does.  4..64 levels. */
int icar_hip_wsm6_init(icar_hip_ctx *ctx);
int icar_hip_wsm6(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte);
/* process_halo's strips (src/physics/mp_driver.f90:609-658) in ONE sequence of launches over up to 4 non-overlapping tiles
 * {its,ite,jts,jte} (as icar_hip_mp_tiles returns them), like icar_hip_thompson_tiles / icar_hip_mp_simple_tiles */
int icar_hip_wsm6_tiles(icar_hip_ctx *ctx, float dt, int ntiles, const int tiles[][4], int kts, int kte);

/* ---- P1: the simple boundary-layer scheme (HP96; src/physics/pbl_simple.f90, src/physics/pbl_driver.f90) ----------------
 * icar_hip_pbl_simple == simple_pbl(th, qv, cloud, ice, qrain, qsnow, u_mass, v_mass, exner, density, z, dz_mass, terrain,
 *     land_mask, its, ite, jts, jte, kts, kte, dt) (pbl_simple.f90:69-141 with pbl_diffusion :165-211) on the context's
 *     POTENTIAL_TEMPERATURE, WATER_VAPOR, CLOUD_WATER, CLOUD_ICE, RAIN, SNOW (mixed in place), U_MASS, V_MASS, EXNER, DENSITY, Z,
 *     DZ_MASS, TERRAIN and LAND_MASK (never uploaded = all land).  Bit-identical to the compiled reference, including its
 *     quirks: the explicit diffusion of a row j takes ceiling(2 maxval(Kq/dz)) sub-steps over its:ite of THAT CALL, so the
 *     result depends on how a domain is cut into tiles; graupel and the number concentrations are not mixed; the level
 *     kte+1 only receives the top flux; temperature and density are not re-diagnosed.  kte is lowered to kme-1 (:92); a
 *     call that leaves no half level (one level) is an error, and so are more than 1024 levels.
 * icar_hip_pbl_configure: options%physics%boundarylayer -- 0, 1 (kPBL_BASIC: pbl_driver.f90 has no branch for it, nothing
 *     runs) or ICAR_PBL_SIMPLE = kPBL_SIMPLE (icar_constants.f90:355); 3 (kPBL_YSU) is refused: it needs pbl_init's arrays, which an
 *     option setter has not built -- icar_hip_pbl_init (P2) selects it.  With the scheme
 *     configured icar_hip_substep / _step / _step_n call pbl between diagnostic_update and the microphysics
 *     (time_step.f90:494) when dt > 1e-3 (:483).  Kept out of icar_hip_step_config so that the struct keeps its layout.
 * icar_hip_pbl == pbl(domain, options, dt) (pbl_driver.f90:197-221) with the tile bounds of icar_hip_step_configure.
 * icar_hip_pbl_nsubsteps: the sub-step count of every row jms..jme of the last call (0 outside its jts..jte), for tests and
 *     measurements; no counterpart in the reference (a local of pbl_diffusion). */
enum { ICAR_PBL_SIMPLE = 2 };
int icar_hip_pbl_simple(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_hip_pbl_configure(icar_hip_ctx *ctx, int boundarylayer);
int icar_hip_pbl(icar_hip_ctx *ctx, float dt);
int icar_hip_pbl_nsubsteps(icar_hip_ctx *ctx, int *nsubsteps, int nrows);

/* ---- P2: the YSU boundary-layer scheme (src/physics/pbl_ysu.f90, src/utilities/pbl_utilities.f90, src/physics/pbl_driver.f90) -------
 * icar_hip_pbl_init == pbl_init(domain, options) (pbl_driver.f90:106-195).  boundarylayer 0, 1, 2: what icar_hip_pbl_configure does.
 *     ICAR_PBL_YSU = kPBL_YSU (icar_constants.f90): the YSU branch :127-194 from the context's Z, TERRAIN, ROUGHNESS_Z0 and LAND_MASK (a
 *     missing upload is an error that names the field): ICAR_YSU_Z_ATM = z(:,kts,:) - terrain, ICAR_YSU_GZ1OZ0 = log(z_atm /
 *     roughness_z0), ICAR_YSU_ZOL = 10, ICAR_YSU_HOL = 1000, the six tendencies and the scheme's results zeroed over the memory; on the
 *     first call it allocates the slot's arrays (ICAR_YSU_*) and the column workspace, 19 arrays x min(kme - kms + 1, 129) levels x
 *     min(nx ny, 131072) columns of REAL(4); then it selects the scheme.  The value is looked at before the context.
 * icar_hip_ysu_sfc == pbl_driver.f90:227-254 alone, over the whole memory: ICAR_YSU_WINDSPD = sqrt(u_10m**2 + v_10m**2) with
 *     `where(windspd==0) windspd=1e-5`, ICAR_YSU_RI = calc_Richardson_nr (atm_utilities.f90:1131-1139) from TEMPERATURE(:,1,:),
 *     SKIN_TEMPERATURE and z_atm, then da_sfc_wtq (pbl_utilities.f90:69-544) -> ICAR_YSU_PSIM, _PSIH, _REGIME from SURFACE_PRESSURE,
 *     ICAR_YSU_GROUND_SURF_TEMPERATURE (domain%ground_surf_temperature has no field id: upload it here; 0 until then), PRESSURE,
 *     TEMPERATURE, U_MASS, V_MASS of level 1, z_atm, ROUGHNESS_Z0, LAND_MASK, USTAR and the dx of icar_hip_step_configure.  As the driver
 *     writes it, da_sfc_wtq's qs is CLOUD_WATER(:,1,:) and its tg the ground temperature, while ysu gets the skin temperature.  Its
 *     u10, v10, t2, q2 are dummies nothing reads and are not computed.  A cell with USTAR <= 0 gets the friction velocity the
 *     reference computes before it has seen a positive one (its use_ust_wrf is a SAVEd variable: such a cell otherwise depends on
 *     the cell visited before it).
 * icar_hip_ysu == `call ysu(...)` (pbl_driver.f90:257-323; pbl_ysu.f90:16-262 with ysu2d :266-1152 and tridin :1154-1234) alone on
 *     its..ite, jts..jte and the levels kts..kte-1 (kte is lowered by one here, as the driver lowers it): from U_MASS, V_MASS,
 *     TEMPERATURE (as diagnostic_update left it), WATER_VAPOR, CLOUD_WATER, CLOUD_ICE, PRESSURE, PRESSURE_INTERFACE, EXNER, DZ_INTERFACE,
 *     SURFACE_PRESSURE, ROUGHNESS_Z0, USTAR, LAND_MASK, SENSIBLE_HEAT, LATENT_HEAT / LH_vaporization, SKIN_TEMPERATURE, U_10M, V_10M and
 *     icar_hip_ysu_sfc's results -> ICAR_YSU_HPBL, _KPBL, _HOL, _EXCH_H (levels kts..kte-2) and the six tendencies ICAR_YSU_TEND_*
 *     (levels kts..kte-1), LEFT IN PLACE.  Bit-identical to the compiled reference.  Refused before any launch: kts /= 1 (ysu2d names
 *     level 1 literally), fewer than 3 levels kts..kte (with one scheme level hpbl reads za(i,0), pbl_ysu.f90:655), more than 129.
 * icar_hip_pbl (P1) == the whole YSU branch of pbl (:223-354) when YSU was initialised: icar_hip_ysu_sfc, icar_hip_ysu on the tile of
 *     icar_hip_step_configure, then over the whole memory x = x + tend dt for WATER_VAPOR, CLOUD_WATER, POTENTIAL_TEMPERATURE, CLOUD_ICE
 *     (where the tendency is 0 -- the top level, the halo -- x + 0: the identity except that -0.0 becomes +0.0) and the six
 *     tendencies to 0.  The u / v tendencies are computed and thrown away, as in the reference (the statements applying them are
 *     commented out there).  icar_hip_substep / _step / _step_n call it in the pbl slot (time_step.f90:494) when dt > 1e-3.
 * icar_hip_ysu_upload / _download: the slot's own arrays by ICAR_YSU_* (they have no field id); count is checked against the array's
 *     size: (nx,ny), (nx,nz,ny) for ICAR_YSU_EXCH_H and the tendencies; REAL(4) but ICAR_YSU_KPBL, which is INTEGER(4). */
enum { ICAR_PBL_YSU = 3 };
enum icar_hip_ysu_array {
    ICAR_YSU_GROUND_SURF_TEMPERATURE = 0,   /* domain%ground_surf_temperature%data_2d (input)                     */
    ICAR_YSU_HPBL = 1,             /* domain%hpbl%data_2d: boundary-layer height (m)                              */
    ICAR_YSU_KPBL = 2,             /* domain%kpbl  INTEGER(4): level of the boundary-layer top                    */
    ICAR_YSU_EXCH_H = 3,           /* domain%coeff_heat_exchange_3d%data_3d (nx,nz,ny)                            */
    ICAR_YSU_PSIM = 4,             /* pbl_driver.f90's psim, psih, regime, Ri, windspd of the last call           */
    ICAR_YSU_PSIH = 5,
    ICAR_YSU_REGIME = 6,
    ICAR_YSU_RI = 7,
    ICAR_YSU_WINDSPD = 8,
    ICAR_YSU_HOL = 9,              /* pbl_driver.f90's hol (1000 after pbl_init), zol (10, never changed)         */
    ICAR_YSU_ZOL = 10,
    ICAR_YSU_GZ1OZ0 = 11,          /* pbl_init's gz1oz0 and z_atm                                                 */
    ICAR_YSU_Z_ATM = 12,
    ICAR_YSU_TEND_TH = 13,         /* domain%tend%th_pbl, %qv_pbl, %qc_pbl, %qi_pbl, %u, %v (nx,nz,ny)            */
    ICAR_YSU_TEND_QV = 14,
    ICAR_YSU_TEND_QC = 15,
    ICAR_YSU_TEND_QI = 16,
    ICAR_YSU_TEND_U = 17,
    ICAR_YSU_TEND_V = 18,
    ICAR_YSU_N = 19
};
int icar_hip_pbl_init(icar_hip_ctx *ctx, int boundarylayer);
int icar_hip_ysu_sfc(icar_hip_ctx *ctx);
int icar_hip_ysu(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_hip_ysu_upload(icar_hip_ctx *ctx, int which, const void *host, size_t count);
int icar_hip_ysu_download(icar_hip_ctx *ctx, int which, void *host, size_t count);

/* ---- R1: the simple radiation scheme (src/physics/ra_simple.f90, src/physics/ra_driver.f90) --------------------------------
 * icar_hip_ra_simple == ra_simple(theta, pii, qv, qc, qs + qi + qg, qr, p, swdown, lwdown, cloud_cover, lat, lon, date, options,
 *     dt, ims..kme, its, ite, jts, jte, kts, kte, F_runlw) (ra_simple.f90:191-272 with calc_solar_elevation :148-189, cloudfrac
 *     :122-146, shortwave :84-103, longwave :105-120 and relative_humidity, atm_utilities.f90:306-326) on the context's
 *     POTENTIAL_TEMPERATURE (cooled in place when runlw), EXNER, WATER_VAPOR, CLOUD_WATER, SNOW + CLOUD_ICE + GRAUPEL (the sum
 *     ra_driver.f90:270-272 passes), RAIN, PRESSURE, LATITUDE, LONGITUDE -> SHORTWAVE, LONGWAVE, CLOUD_FRACTION; `date` is the
 *     library clock (icar_hip_model_time) under the anchor of icar_hip_rad_calendar.  Bit-identical to the compiled reference,
 *     including its quirks: CLOUD_FRACTION(ims:ime, j) OUTSIDE its:ite becomes 5e-8 on every row jts..jte (cloudfrac zeroes its
 *     whole result and then floors the whole of it, :132-139); SHORTWAVE / LONGWAVE outside its:ite are an uninitialised
 *     function result in the reference and are left untouched here; temperature and density are not re-diagnosed after the
 *     cooling.  T_air and rh are means over kts..kts+4: fewer than 5 levels (the reference reads out of bounds) is an error,
 *     "ra_simple: at least 5 levels", before any launch.  cos_lat_m / sin_lat_m of ra_simple_init (:62-81) are kept in the
 *     context and made again when the scheme is configured or LATITUDE is uploaded.
 * icar_hip_rad_configure: options%physics%radiation -- 0, 1 (kRA_BASIC: ra_driver.f90 has no branch for it, nothing runs) or
 *     ICAR_RA_SIMPLE = kRA_SIMPLE (icar_constants.f90); 3 (kRA_RRTMG) is refused: not built.  With the scheme configured
 *     icar_hip_substep / _step / _step_n call rad after diagnostic_update and before pbl and the microphysics
 *     (time_step.f90:488) when dt > 1e-3 (:483).  Kept out of icar_hip_step_config so that the struct keeps its layout.
 * icar_hip_rad_calendar: what Time_type%day_of_year / %year_fraction (time_obj.f90:404-480) need of domain%model_time.
 *     calendar: 0 gregorian, 1 noleap, 2 360-day; year_start_seconds: the value of the library clock at 1 January 00:00 of the
 *     year that contains the model time; year_days / next_year_days: the lengths of that year and of the next.  At the start of
 *     each sub-step D = (model_time - year_start_seconds) / 86400 in FP64, rolled into the next year once when D >= year_days;
 *     day_of_year(lon) = (float)(D + (double)offset(lon)); year_fraction(lon) = (float)((D + offset) / year_days) (gregorian),
 *     day_of_year / 365.0f (noleap), / 360.0f (360-day), then mod(., 1.0).  The reference does this sum in REAL(16) from a
 *     modified Julian day; time_obj.f90 cannot be compiled here, so THIS PART IS NOT PINNED to the compiled reference (FP64
 *     and REAL(16) can differ in the last bit of the REAL(4) day of the year when D + offset lies within 2^-53 of a tie).
 * icar_hip_rad == rad(domain, options, dt) (ra_driver.f90:197-285) with the tile bounds of icar_hip_step_configure; an error
 *     when radiation = 2 and no calendar was set. */
enum { ICAR_RA_SIMPLE = 2 };
int icar_hip_ra_simple(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte, int runlw);
int icar_hip_rad_configure(icar_hip_ctx *ctx, int radiation);
int icar_hip_rad_calendar(icar_hip_ctx *ctx, int calendar, double year_start_seconds, double year_days, double next_year_days);
int icar_hip_rad(icar_hip_ctx *ctx, float dt);

/* ---- L1: the surface-flux slot (src/physics/lsm_driver.f90 for landsurface = kLSM_BASIC, src/physics/water_simple.f90) -----------
 * icar_hip_lsm_configure: lsm_init (lsm_driver.f90:522-611, :991-1000) -- options%physics%landsurface / %watersurface and
 *     options%lsm_options%update_interval (integer seconds, default 300), %sh_feedback_fraction (0.625), %lh_feedback_fraction (1.0),
 *     %sfc_layer_thickness (400 m); resets last_model_time to its sentinel -999 (:1000) and forgets apply_fluxes' nz.
 *     landsurface: 0 (lsm returns at once, :1014, whatever watersurface is) or 1 = kLSM_BASIC (fluxes prescribed by the host or
 *     computed over open water, applied to the atmosphere).  2 (kLSM_SIMPLE) is refused as the reference refuses it: "Simple LSM
 *     not settup, choose a different LSM options" (:615); 3 (kLSM_NOAH) is refused here ("not built" behind this entry point): it
 *     needs the tables and options%lsm_options, which icar_hip_lsm_init (L2) takes; 4 (kLSM_NOAHMP) is refused: not built.  watersurface:
 *     0, 1 (kWATER_BASIC: nothing runs, :1038-1050) or ICAR_WATER_SIMPLE = kWATER_SIMPLE; 3 (kWATER_LAKE) is refused: not built.
 *     The values are looked at before the context.  QSFC = water_vapor(:,kms,:) (:568) is taken here when water_vapor is on the
 *     device, else at the first icar_hip_water_simple.  Kept out of icar_hip_step_config so that the struct keeps its layout.
 * icar_hip_diag_10m == time_step.f90:143-161 of diagnostic_update: u_10m, v_10m and ustar on ims+1:ime-1, jms+1:jme-1 from
 *     ROUGHNESS_Z0, Z, TERRAIN, U_MASS, V_MASS (u_10m = (u_mass currw) lastw, the product rounded in between as it passes
 *     through domain%ustar).  icar_hip_diagnostic_update and the step entry points call it behind the mass-point winds whenever
 *     ROUGHNESS_Z0 has been uploaded (the reference's `associated` test); without it nothing new is issued.
 * icar_hip_water_simple == the gated block of lsm with watersurface = kWATER_SIMPLE (lsm_driver.f90:1028-1073): windspd =
 *     sqrt(u_10m**2 + v_10m**2), `where(wind==0) wind=1e-5` (the one visible effect of calc_exchange_coefficient on this path:
 *     its result CHS is read by Noah alone and is NOT built), then water_simple (water_simple.f90:83-136) on 2..nx-1, 2..ny-1 of
 *     the MEMORY rectangle where LAND_MASK == kLC_WATER: QSFC = 0.98 sat_mr(SST, SURFACE_PRESSURE), ROUGHNESS_Z0 = 8e-6 /
 *     max(USTAR, 1e-7) (read by the next icar_hip_diag_10m), SENSIBLE_HEAT, QFX, LATENT_HEAT = QFX LH_vaporization,
 *     SKIN_TEMPERATURE = SST, from TEMPERATURE(:,kms,:), WATER_VAPOR(:,kms,:) and z_atm = Z(:,kms,:) - TERRAIN.  Land cells keep
 *     what the host uploaded.
 * icar_hip_apply_fluxes == apply_fluxes(domain, dt) (lsm_driver.f90:361-423): SENSIBLE_HEAT and LATENT_HEAT into
 *     POTENTIAL_TEMPERATURE and WATER_VAPOR of its:ite, jts:jte on the levels kts .. kts+nz with DENSITY, EXNER, DZ_INTERFACE, then
 *     where(qv < 1e-10) qv = 1e-10 over the WHOLE array.  nz is the last level (its absolute index) at which the running sum of
 *     maxval(dz_interface(:,k,:)) over THIS CONTEXT'S MEMORY is below sfc_layer_thickness: found once, again when DZ_INTERFACE
 *     is uploaded or the slot reconfigured; a tiling can find another nz than one image does, in the reference and here.  The
 *     loop runs one level past nz (with kts > kms further still); where that passes kte the reference reads out of bounds and
 *     this call is refused before any launch ("the surface layer reaches kte").
 * icar_hip_lsm == lsm(domain, options, dt) (:1005-1554): the gate on the library clock (:1016-1023: REAL(8), the block runs when
 *     model_time - last_model_time >= update_interval), icar_hip_water_simple inside it when watersurface = 2, then
 *     icar_hip_apply_fluxes on the tile of icar_hip_step_configure, every call.  icar_hip_substep / _step / _step_n call it
 *     between rad and pbl (time_step.f90:491) when dt > 1e-3.
 * icar_hip_lsm_layers: apply_fluxes' nz for the configured tile's kts..kte, for tests and logs. */
enum { ICAR_LSM_BASIC = 1, ICAR_WATER_SIMPLE = 2 };
int icar_hip_lsm_configure(icar_hip_ctx *ctx, int landsurface, int watersurface, int update_interval, float sh_feedback_fraction,
                           float lh_feedback_fraction, float sfc_layer_thickness);
int icar_hip_diag_10m(icar_hip_ctx *ctx);
int icar_hip_water_simple(icar_hip_ctx *ctx);
int icar_hip_apply_fluxes(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte, int kts, int kte);
int icar_hip_lsm(icar_hip_ctx *ctx, float dt);
int icar_hip_lsm_layers(icar_hip_ctx *ctx, int *nz);

/* ---- L2: the Noah land-surface model (src/physics/lsm_noahlsm.f90, src/physics/lsm_noahdrv.f90, src/physics/lsm_driver.f90) -----------
 * icar_hip_noah_tables: the three tables as SOIL_VEG_GEN_PARM (lsm_noahdrv.f90:1199-1432) parsed them, copied to the device: a host
 *     calls the reference's own SOIL_VEG_GEN_PARM(LU_Categories, "STAS") and hands module_sf_noahlsm's arrays over, each with the
 *     module's extent (NLUS = 50, NSLTYPE = 30, NSLOPE = 30); there is no table parser here.  Comes first: the ICAR_NOAH_* arrays
 *     exist from here on.  Refused before the context: LUCATS / SLCATS / SLPCATS outside the extents, NROTBL outside 0 .. 4, BARE.
 * icar_hip_lsm_init == lsm_init(domain, options) (lsm_driver.f90:522-711).  landsurface 0, 1, 2: what icar_hip_lsm_configure does
 *     (noah may be NULL).  ICAR_LSM_NOAH = kLSM_NOAH: the Noah part :619-711.  The domain's arrays it reads must have been uploaded by
 *     ICAR_NOAH_*: VEG_TYPE, SOIL_TYPE, VEGFRAC (domain%vegetation_fraction(:,1,:)), ALBEDO (domain%albedo(:,1,:)),
 *     SOIL_DEEP_TEMPERATURE, SOIL_WATER_CONTENT, SOIL_TEMPERATURE (a missing one is an error that names it); SNOW_WATER_EQUIVALENT,
 *     SNOW_HEIGHT, CANOPY_WATER and LAI are 0 until uploaded, as domain_t allocates them.  It gives the module's own arrays
 *     allocate_noah_data's values (:425-520: SMSTAV 0.5, SNOALB 0.8, QGH 0.02, ALBBCK 0.17, EMISS 0.99, SHDMIN 0, SHDMAX 100, SH2O 0.25,
 *     the rest 0; EMBCK = 0.99 is overwritten by SFLX before it is read and has no array), applies the two floors of :674-675
 *     (SOIL_TEMPERATURE >= 200, SOIL_WATER_CONTENT >= 0.0001), runs LSM_NOAH_INIT's per-cell part (lsm_noahdrv.f90:1095-1188: SNOALB from
 *     MAXALB, SH2O from FRH2O where the soil is below 273.149 K, SNOW_HEIGHT = 0.005 SNOW_WATER_EQUIVALENT unless fndsnowh -- over the
 *     WHOLE MEMORY, where the reference takes the tile its .. min(ite, ide-1) of domain%grid (:550-553, :705) and leaves an image's halo
 *     cells at SH2O = 0.25, SNOALB = 0.8: lsm_noah reads no neighbour, so no owned cell differs) with CANOPY_WATER restored afterwards (:672, :707), sets CQS2 = 0.01 (:708) and LAND_MASK = kLC_WATER where VEG_TYPE
 *     is water_category or lake_category (:710; a LAND_MASK never uploaded starts as all land).  A cell of the memory whose VEG_TYPE /
 *     SOIL_TYPE is outside 1 .. LUCATS / 1 .. SLCATS is an error (the reference would read table rows that were never filled), found before
 *     anything is written: every refusal leaves the context as it was.  New categories or new tables afterwards need a new icar_hip_lsm_init.  The values are looked at before the context: 4 (kLSM_NOAHMP) and
 *     watersurface = 3 (kWATER_LAKE) are refused: not built; monthly_vegfrac / monthly_albedo are refused: not built (the host uploads
 *     the month's VEGFRAC / ALBEDO itself).
 * icar_hip_lsm_noah == `call lsm_noah(...)` (lsm_driver.f90:1210-1278; lsm_noahdrv.f90:36-1018 with SFLX and its 27 helpers,
 *     lsm_noahlsm.f90:64-4228) alone on its..ite, jts..jte with DT = lsm_dt and the constants of allocate_noah_data (four soil layers of
 *     0.1, 0.3, 0.6, 1.0 m, ITIMESTEP = 1, XICE = 0, MYJ / FRPCPN / RDLAI2D / USEMONALB / UA_PHYS false): from WATER_VAPOR, TEMPERATURE (level 1),
 *     PRESSURE_INTERFACE (levels 1, 2), SHORTWAVE, LONGWAVE, LAND_MASK, the ICAR_NOAH_* inputs and state -> SKIN_TEMPERATURE, SENSIBLE_HEAT,
 *     LATENT_HEAT, QFX, QSFC, ROUGHNESS_Z0 (ZNT) and the ICAR_NOAH_* state.  RAINBL is ICAR_NOAH_CURRENT_PRECIPITATION, CHS ICAR_NOAH_CHS, Ri
 *     ICAR_NOAH_RI, QGH ICAR_NOAH_QGH: the statements of lsm() that make them (:1028-1030, :1181-1187, :1207) are NOT built, the host uploads
 *     them (CHS is required; the others keep lsm_init's values).  Bit-identical to the compiled reference in every cell that runs SFLX
 *     and every water cell (the every-call block lsm_noahdrv.f90:623-650).  A land-ice cell (VEG_TYPE == ice_category, :887-901) gets
 *     what the reference defines there (SOIL_WATER_CONTENT = SH2O = SMCREL = 1, LAI = 0.01, SOIL_TOTALMOISTURE = 0, the re-derived snow
 *     height, ...); ALBEDO, ZNT, the fluxes, QSFC, POTEVP, NOAHRES, SMSTAV, SFCRUNOFF, ACSNOM, SNOPCX and FLX4 / FVB / FBUR / FGSN are
 *     left as they are: the reference stores locals there that only SFLX sets, i.e. the values of the cell visited before.  Refused:
 *     kts /= 1 or a single level (lsm_noah names level 1 literally), a tile outside the memory.
 * icar_hip_lsm (L1) with Noah initialised answers that the Noah branch of lsm() is not built and names icar_hip_lsm_noah; icar_hip_substep /
 *     _step / _step_n answer the same before they issue anything.
 * icar_hip_noah_upload / _download: the arrays by ICAR_NOAH_*: (nx,ny) REAL(4), but VEG_TYPE / SOIL_TYPE INTEGER(4) (nx,ny) and the four
 *     soil arrays REAL(4) (nx,4,ny). */
enum { ICAR_LSM_NOAH = 3 };
enum icar_hip_noah_array {
    ICAR_NOAH_VEG_TYPE = 0,                /* domain%veg_type   INTEGER(4)                                        */
    ICAR_NOAH_SOIL_TYPE = 1,               /* domain%soil_type  INTEGER(4)                                        */
    ICAR_NOAH_VEGFRAC = 2,                 /* lsm_driver.f90's VEGFRAC [%]                                         */
    ICAR_NOAH_SOIL_DEEP_TEMPERATURE = 3,   /* domain%soil_deep_temperature%data_2d (TMN)                           */
    ICAR_NOAH_SHDMIN = 4,                  /* the module's own arrays, named as lsm_driver.f90 names them          */
    ICAR_NOAH_SHDMAX = 5,
    ICAR_NOAH_SNOALB = 6,
    ICAR_NOAH_QGH = 7,
    ICAR_NOAH_CHS = 8,
    ICAR_NOAH_CQS2 = 9,
    ICAR_NOAH_RI = 10,
    ICAR_NOAH_CURRENT_PRECIPITATION = 11,  /* current_precipitation (:1207) [kg m-2 per lsm_dt]                    */
    ICAR_NOAH_GROUND_HEAT_FLUX = 12,       /* domain%ground_heat_flux%data_2d                                      */
    ICAR_NOAH_SMSTAV = 13,
    ICAR_NOAH_SOIL_TOTALMOISTURE = 14,     /* domain%soil_totalmoisture%data_2d (SMSTOT)                           */
    ICAR_NOAH_SFCRUNOFF = 15,
    ICAR_NOAH_UDRUNOFF = 16,
    ICAR_NOAH_ALBEDO = 17,
    ICAR_NOAH_ALBBCK = 18,
    ICAR_NOAH_Z0 = 19,
    ICAR_NOAH_EMISS = 20,
    ICAR_NOAH_SNOWC = 21,
    ICAR_NOAH_SNOW_WATER_EQUIVALENT = 22,  /* domain%snow_water_equivalent%data_2d [kg m-2]                        */
    ICAR_NOAH_SNOW_HEIGHT = 23,            /* domain%snow_height%data_2d [m]                                       */
    ICAR_NOAH_CANOPY_WATER = 24,           /* domain%canopy_water%data_2d                                          */
    ICAR_NOAH_CHS2 = 25,
    ICAR_NOAH_CHKLOWQ = 26,
    ICAR_NOAH_LAI = 27,                    /* domain%lai%data_2d                                                   */
    ICAR_NOAH_SNOTIME = 28,
    ICAR_NOAH_ACSNOM = 29,
    ICAR_NOAH_ACSNOW = 30,
    ICAR_NOAH_SNOPCX = 31,
    ICAR_NOAH_POTEVP = 32,
    ICAR_NOAH_NOAHRES = 33,
    ICAR_NOAH_FLX4 = 34,
    ICAR_NOAH_FVB = 35,
    ICAR_NOAH_FBUR = 36,
    ICAR_NOAH_FGSN = 37,
    ICAR_NOAH_SOIL_WATER_CONTENT = 38,     /* domain%soil_water_content%data_3d (nx,4,ny) (SMOIS)                  */
    ICAR_NOAH_SOIL_TEMPERATURE = 39,       /* domain%soil_temperature%data_3d (nx,4,ny) (TSLB)                     */
    ICAR_NOAH_SH2O = 40,                   /* (nx,4,ny)                                                            */
    ICAR_NOAH_SMCREL = 41,                 /* (nx,4,ny)                                                            */
    ICAR_NOAH_N = 42
};
/* module_sf_noahlsm's public table variables (lsm_noahlsm.f90:26-54); arrays of NLUS = 50, NSLTYPE = 30, NSLOPE = 30 elements */
typedef struct icar_hip_noah_tables_t {
    const int *nrotbl;
    const float *snuptbl, *rstbl, *rgltbl, *hstbl, *maxalb, *emissmintbl, *emissmaxtbl, *laimintbl, *laimaxtbl, *z0mintbl, *z0maxtbl,
        *albedomintbl, *albedomaxtbl;
    const float *bb, *drysmc, *f11, *maxsmc, *refsmc, *satpsi, *satdk, *satdw, *wltsmc, *qtz;
    const float *slope_data;
    float topt_data, cmcmax_data, cfactr_data, rsmax_data;
    float sbeta_data, fxexp_data, csoil_data, salp_data, refdk_data, refkdt_data, frzk_data, zbot_data, lvcoef_data;
    int bare, lucats, slcats, slpcats;
} icar_hip_noah_tables_t;
/* options%lsm_options as lsm_init reads them for Noah (lsm_driver.f90:633-651, :1280) */
typedef struct icar_hip_noah_options_t {
    int urban_category, ice_category, water_category, lake_category;
    int monthly_vegfrac, monthly_albedo;      /* must be 0: not built */
    int fndsnowh;                             /* FNDSNOWH (:633-642): 1 = SNOW_HEIGHT was read from the input, 0 = derive it from the snow water */
    float max_swe;
} icar_hip_noah_options_t;
int icar_hip_noah_tables(icar_hip_ctx *ctx, const icar_hip_noah_tables_t *tables);
int icar_hip_lsm_init(icar_hip_ctx *ctx, int landsurface, int watersurface, int update_interval, float sh_feedback_fraction,
                      float lh_feedback_fraction, float sfc_layer_thickness, const icar_hip_noah_options_t *noah);
int icar_hip_lsm_noah(icar_hip_ctx *ctx, float lsm_dt, int its, int ite, int jts, int jte);
int icar_hip_noah_upload(icar_hip_ctx *ctx, int which, const void *host);
int icar_hip_noah_download(icar_hip_ctx *ctx, int which, void *host);

/* ---- L3: the Noah branch of lsm() around the call (src/physics/lsm_driver.f90 with landsurface = kLSM_NOAH) ------------------------------
 * Nothing below changes what L1 and L2 do until icar_hip_lsm_noah_couple has been called.
 * icar_hip_lsm_noah_couple == what lsm_init does for Noah beside the part of icar_hip_lsm_init, called after
 *     icar_hip_lsm_init(.., ICAR_LSM_NOAH, ..): Z0 = roughness_z0 (lsm_driver.f90:566, into ICAR_NOAH_Z0), current_precipitation = 0
 *     (:583-587; windspd = 3 is overwritten at :1028 before anything reads it and has no array), CHS = 0.01 and CHS2 = 0.01 (:592-596),
 *     RAINBL = accumulated_precipitation (:602-603, REAL(8)), temperature_2m = temperature(:,kms,:) and humidity_2m = water_vapor(:,kms,:)
 *     (:610-611), z_atm = z(:,kts,:) - terrain (:992), lnz_atm_term and base_exchange_term (:993-997) with exchange_term = 1.  That is the
 *     only value lsm_init ever sets (:535): calc_mahrt_holtslag_exchange_coefficient and F2_formula (:269-297) are unreachable and are NOT
 *     built.  Needs ROUGHNESS_Z0, Z, TERRAIN, TEMPERATURE, WATER_VAPOR, SURFACE_PRESSURE and either U_10M / V_10M or U_MASS / V_MASS (then
 *     icar_hip_diag_10m runs once); a missing one is an error that names it.  ICAR_F_PRECIPITATION never uploaded is the zeros domain_t
 *     allocates.  Refused before anything is written, the context left as it was: Noah not initialised (or new tables / categories / another
 *     icar_hip_lsm_init or _lsm_configure since), a step tile with kts /= kms.  A later icar_hip_lsm_init / icar_hip_lsm_configure drops the
 *     coupling: icar_hip_lsm and the step entry points refuse Noah again until the next icar_hip_lsm_noah_couple.
 * icar_hip_lsm (L1) with the coupling made == lsm(domain, options, dt) for kLSM_NOAH (:1005-1554): the gate on the library clock
 *     (:1016-1023, lsm_dt the REAL(8) difference stored into a REAL(4)); inside it windspd (:1028) and calc_exchange_coefficient (:244-265)
 *     over the memory rectangle into ICAR_NOAH_RI / ICAR_NOAH_CHS; water_simple when watersurface = 2 (:1051-1073); windspd floored at 1,
 *     CHS = CHS * windspd, CHS2 = CHS, CQS2 = CHS (:1144-1147); QGH = sat_mr(temperature_2m, surface_pressure) where land_mask == kLC_LAND
 *     (:1181-1187, sat_mr of atm_utilities.f90:523-560); current_precipitation = accumulated_precipitation - RAINBL (:1207, a REAL(8)
 *     difference rounded to REAL(4); domain%rain_fraction, :1208, is allocated only with the bias-correction options, is NOT built and cannot
 *     be supplied); lsm_noah (:1210-1278) on the tile of icar_hip_step_configure; then over the memory rectangle the max_swe clamp (:1280),
 *     the exchange terms from the new roughness_z0 (:1282-1286), longwave_up (:1289), RAINBL = accumulated_precipitation (:1290; rain_bucket,
 *     :1291, feeds only a commented-out term and has no array); soil_totalmoisture (:1524-1527, which overwrites what lsm_noah stored, land-ice
 *     cells included); surface_diagnostics (:299-359) on its..ite, jts..jte.  Of surface_diagnostics only the bulk arm (:337-352) is built: for
 *     Noah lsm_var_request (:119-129) allocates temperature_2m_veg but not temperature_2m_bare, so `associated(T2bare)` is false and the veg
 *     and bare arms are dead.  Then, every call, icar_hip_apply_fluxes (:1550-1552).  The host uploads neither CHS, Ri, QGH nor
 *     current_precipitation and keeps none of these statements.  icar_hip_substep / _step / _step_n run this in their lsm slot
 *     (time_step.f90:491).
 * icar_hip_lsm_upload / _download: the arrays of enum icar_hip_lsm_array, (nx,ny) REAL(4) but RAINBL REAL(8) -- what a restart hands over
 *     beside the ICAR_NOAH_* arrays (upload them after icar_hip_lsm_noah_couple, which rewrites all but LONGWAVE_UP). */
enum icar_hip_lsm_array {
    ICAR_LSM_TEMPERATURE_2M = 0,           /* domain%temperature_2m%data_2d                                        */
    ICAR_LSM_HUMIDITY_2M = 1,              /* domain%humidity_2m%data_2d                                           */
    ICAR_LSM_LONGWAVE_UP = 2,              /* domain%longwave_up%data_2d                                           */
    ICAR_LSM_RAINBL = 3,                   /* lsm_driver.f90's RAINBL  REAL(8)                                     */
    ICAR_LSM_Z_ATM = 4,
    ICAR_LSM_LNZ_ATM_TERM = 5,
    ICAR_LSM_BASE_EXCHANGE_TERM = 6,
    ICAR_LSM_N = 7
};
int icar_hip_lsm_noah_couple(icar_hip_ctx *ctx);
int icar_hip_lsm_upload(icar_hip_ctx *ctx, int which, const void *host);
int icar_hip_lsm_download(icar_hip_ctx *ctx, int which, void *host);

/* ---- C1: the convection slot (src/physics/cu_driver.f90 with convection = kCU_BMJ, src/physics/cu_bmj.f90) ---------------------------
 * icar_hip_cu_configure: init_convection (cu_driver.f90:97-253) -- options%physics%convection and options%cu_options.
 *     convection: 0 (convect returns at once, :264) or ICAR_CU_BMJ = kCU_BMJ (icar_constants.f90:345).  1 (kCU_TIEDTKE) is refused here:
 *     it needs znu, which icar_hip_cu_init (C2) takes.  4 (kCU_NSAS) is refused here ("not built" behind this entry point): it needs dx,
 *     which icar_hip_convection_init (C3) takes.  2 (kCU_SIMPLE) is refused: cu_driver.f90 has no branch for it and cu_simple.f90 is not among the
 *     reference's objects; 3 (kCU_KAINFR) likewise: its branch in cu_driver.f90 is commented out and cu_kf.f90 is not built.
 *     stochastic_cu: ICAR_CU_NO_STOCHASTIC = kNO_STOCHASTIC (-9999); anything else draws from random_number in the reference
 *     (:287-295) and is refused.  tendency_fraction (default 1.0) and the four fractions of qv, qc, th, qi (negative = inherit
 *     tendency_fraction, options_obj.f90:1646-1649).  The values are looked at before the context.  With convection = 5 the call
 *     allocates the slot's own arrays (ICAR_CU_*: CLDEFI = AVGEFI = 0.6 as BMJINIT leaves it, the rest 0), builds BMJINIT's nine
 *     lookup tables on the host (SPLINE and all, with cp = 1012 and r_d = 287 as :236-237 passes them) into device memory and
 *     allocates the column workspace: 16 arrays x min(kme - kms, 128) levels x min(nx ny, 65536) columns of REAL(4).  Kept out of
 *     icar_hip_step_config so that the struct keeps its layout.
 * icar_hip_cu_bmj == the call of BMJDRV (:434-465) alone on its..ite, jts..jte and the levels kts..kte-1 of
 *     icar_hip_step_configure (kms..kme-1 without one): from TEMPERATURE (as diagnostic_update left it -- NOT recomputed from the
 *     current potential temperature), the current WATER_VAPOR, PRESSURE, PRESSURE_INTERFACE, EXNER, DENSITY, DZ_INTERFACE, LAND_MASK
 *     (never uploaded = all land) and ICAR_CU_CLDEFI -> ICAR_CU_TEND_TH = DTDT / exner, ICAR_CU_TEND_QV = DQDT / (1 - q)**2,
 *     ICAR_CU_RAINCV = PCPCOL 1e3, ICAR_CU_CLDEFI, ICAR_CU_CUTOP, ICAR_CU_CUBOT of those columns; nothing else is touched.  Bit-identical
 *     to the compiled reference.  NOT built: the bmj_rad_feedback block (cu_bmj.f90:267-351: CCLDFRA, QCCONV, QICONV, CONVCLD,
 *     PRATEC) -- those arrays are private to cu_driver.f90, nothing reads them, and the block needs GAMMA() in REAL(4); W0AVG, which
 *     BMJ never reads.  Levels: kts = 1 (BMJDRV's flip KFLIP = KTE+1-K and PSFC = PINT(i,1,j) assume it; with kts = 2 the reference
 *     reads DTDT(1) below its lower bound, cu_bmj.f90:248), at least 3 levels kts..kte (with one scheme level the reference reads
 *     PRSMID(LBOT+1) past the column, :755), at most 129; all refused before any launch.  A trial parcel whose cloud base cannot be
 *     put PONE = 2500 Pa above the lowest level (a column thinner than 25 hPa; the reference reads level LMH+1 there) gets no CAPE.
 * icar_hip_convect == convect(domain, options, dt) (:255-514) on the tile of icar_hip_step_configure: tend%th, tend%qv and RAINCV
 *     zeroed over all i and k of memory on the rows jts..jte (:272-282), icar_hip_cu_bmj, then on those rows and all i, k of memory
 *     x = x + (tend dt) fraction for WATER_VAPOR, CLOUD_WATER, POTENTIAL_TEMPERATURE, CLOUD_ICE whose fraction is > 0 when
 *     tendency_fraction > 0 (BMJ leaves tend%qc and tend%qi at 0: those two get x + 0, the identity except that -0.0 becomes +0.0),
 *     PRECIPITATION (REAL(8)) += RAINCV and ICAR_CU_ACC_CONV_PCP += RAINCV (:483-500).  Column-local on owned columns, in front of
 *     mp(halo=1) and halo_send: an N-image run equals the one-image run in every owned cell.  icar_hip_substep / _step / _step_n
 *     call it between pbl and the microphysics (time_step.f90:509) when dt > 1e-3.
 * icar_hip_cu_reset: CLDEFI = AVGEFI, accumulated_convective_pcp = 0 (a restart of the slot).
 * icar_hip_cu_upload / _download: the slot's own arrays by ICAR_CU_* (they have no field id): REAL(4), (nx,ny) but for the two
 *     tendencies (nx,nz,ny).  icar_hip_cu_tables: QS0(134), SQS(134), PTBL(76,134), THE0(76), STHE(76), TTBL(134,76), THE0Q(152),
 *     STHEQ(152), TTBLQ(440,152) one behind the other, Fortran element order; out may be NULL to query the count. */
enum { ICAR_CU_BMJ = 5 };
#define ICAR_CU_NO_STOCHASTIC (-9999.0f)
enum icar_hip_cu_array {
    ICAR_CU_CLDEFI = 0,            /* cu_driver.f90's CLDEFI: precipitation efficiency, carried from call to call */
    ICAR_CU_ACC_CONV_PCP = 1,      /* domain%accumulated_convective_pcp%data_2d                                   */
    ICAR_CU_RAINCV = 2,            /* cu_driver.f90's RAINCV of the last call (mm)                                */
    ICAR_CU_CUTOP = 3,             /* CUTOP, CUBOT of the last call (level indices as REAL(4))                    */
    ICAR_CU_CUBOT = 4,
    ICAR_CU_TEND_TH = 5,           /* domain%tend%th (nx,nz,ny)                                                   */
    ICAR_CU_TEND_QV = 6,           /* domain%tend%qv (nx,nz,ny)                                                   */
    ICAR_CU_N = 7
};
int icar_hip_cu_configure(icar_hip_ctx *ctx, int convection, float stochastic_cu, float tendency_fraction, float tend_qv_fraction,
                          float tend_qc_fraction, float tend_th_fraction, float tend_qi_fraction);
int icar_hip_cu_bmj(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte);
int icar_hip_convect(icar_hip_ctx *ctx, float dt);
int icar_hip_cu_reset(icar_hip_ctx *ctx);
int icar_hip_cu_upload(icar_hip_ctx *ctx, int which, const void *host);
int icar_hip_cu_download(icar_hip_ctx *ctx, int which, void *host);
int icar_hip_cu_tables(icar_hip_ctx *ctx, float *out, size_t capacity, size_t *count);

/* ---- C2: the Tiedtke scheme in the convection slot (cu_driver.f90 with convection = kCU_TIEDTKE, src/physics/cu_tiedtke.f90) ----------
 * icar_hip_cu_init == init_convection(domain, options) (cu_driver.f90:97-253) with every scheme that is built.  convection 0 or
 *     ICAR_CU_BMJ: exactly icar_hip_cu_configure (znu may be NULL).  ICAR_CU_TIEDTKE = kCU_TIEDTKE (icar_constants.f90): znu is
 *     domain%znu(kms:kme), copied; the call allocates tend%qc, tend%qi, PRATEC and KTYPE (ICAR_TIEDTKE_*, zero as tiedtkeinit leaves
 *     them), the slot's ICAR_CU_* arrays and the column workspace: 25 arrays x (min(kme - kms, 128) + 2) levels x min(nx ny, 65536)
 *     columns of REAL(4), and 16 values per column beside it.  4, 2, 3, a stochastic_cu other than ICAR_CU_NO_STOCHASTIC and a NaN
 *     are refused as by icar_hip_cu_configure; the values are looked at before the context.
 * icar_hip_cu_tiedtke == the call of CU_TIEDTKE (:303-330) alone on its..ite, jts..jte and the levels kts..kte-1 of
 *     icar_hip_step_configure (kms..kme-1 without one), with itimestep = STEPCU = 1: from TEMPERATURE (as diagnostic_update left
 *     it), WATER_VAPOR, CLOUD_WATER, CLOUD_ICE, EXNER, DENSITY, W_REAL (W0AVG without the stochastic term), DZ_INTERFACE, PRESSURE,
 *     PRESSURE_INTERFACE, LAND_MASK (never uploaded = all land; XLAND = 2 where the mask is 0 or 2) and znu -> ICAR_CU_TEND_TH,
 *     ICAR_CU_TEND_QV, ICAR_TIEDTKE_TEND_QC, ICAR_TIEDTKE_TEND_QI, ICAR_CU_RAINCV, ICAR_TIEDTKE_PRATEC and ICAR_TIEDTKE_KTYPE of
 *     those columns; nothing else is touched.  Bit-identical to the compiled reference.  With itimestep = 1 the moisture
 *     convergence PQTE is zero on entry, so no column is ever of KTYPE 1 or 2: convection starts at mid level (CUBASMC, KTYPE 3) or
 *     not at all, and LATENT_HEAT, SENSIBLE_HEAT and the winds are read by nothing that is evaluated (icar_amd/csrc/tiedtke_column.h
 *     has the derivation); tend%u / tend%v (CUDUDV) are not built: convect applies neither (:502-507 is commented out).
 *     `leveltop`, the level above which mid-level convection may not start, is made once per row from the pressure of column its,
 *     as the reference makes it from the first column of its tile row: an N-image run may differ from the one-image run there,
 *     in the reference and here.  Levels: kts = 1, at least 4 levels kts..kte (with two scheme levels the reference reads
 *     PAPH(JL,0), cu_tiedtke.f90:937), at most 129; all refused before any launch.
 * icar_hip_convect / _substep / _step / _step_n run this scheme when icar_hip_cu_init selected it: tend%qc and tend%qi are zeroed
 *     and applied like the other two, and the whole of diagnostic_update, w_real included, precedes convect in the sub-step.
 * icar_hip_tiedtke_upload / _download: the scheme's own arrays by ICAR_TIEDTKE_*: the two tendencies (nx,nz,ny) and PRATEC (nx,ny)
 *     REAL(4), KTYPE (nx,ny) INTEGER(4): the column's final KTYPE (0 or 3). */
enum { ICAR_CU_TIEDTKE = 1 };
enum icar_hip_tiedtke_array {
    ICAR_TIEDTKE_TEND_QC = 0,      /* domain%tend%qc (nx,nz,ny)                                                   */
    ICAR_TIEDTKE_TEND_QI = 1,      /* domain%tend%qi (nx,nz,ny)                                                   */
    ICAR_TIEDTKE_PRATEC = 2,       /* cu_driver.f90's PRATEC of the last call (mm/s)                              */
    ICAR_TIEDTKE_KTYPE = 3,        /* KTYPE of the last call, INTEGER(4)                                          */
    ICAR_TIEDTKE_N = 4
};
int icar_hip_cu_init(icar_hip_ctx *ctx, int convection, float stochastic_cu, float tendency_fraction, float tend_qv_fraction,
                     float tend_qc_fraction, float tend_th_fraction, float tend_qi_fraction, const float *znu);
int icar_hip_cu_tiedtke(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte);
int icar_hip_tiedtke_upload(icar_hip_ctx *ctx, int which, const void *host);
int icar_hip_tiedtke_download(icar_hip_ctx *ctx, int which, void *host);

/* ---- C3: the NSAS scheme in the convection slot (cu_driver.f90 with convection = kCU_NSAS, src/physics/cu_nsas.f90) -------------------
 * icar_hip_convection_init == init_convection(domain, options) (cu_driver.f90:97-253) with every scheme that is built.  convection 0,
 *     ICAR_CU_BMJ and ICAR_CU_TIEDTKE: exactly icar_hip_cu_init (dx ignored).  ICAR_CU_NSAS = kCU_NSAS (icar_constants.f90; :59-73,
 *     :173-202): dx is domain%dx, kept (it decides dx_factor_nsas, :357-361, and is nsas2d's delx); a dx <= 0 or a dx that is not a
 *     number is refused, the values being looked at before the context.  The call allocates tend%qc, tend%qi (zero as nsasinit leaves
 *     them, cu_nsas.f90:2155-2186), PRATEC, HBOT, HTOP and hpbl (ICAR_NSAS_*), the slot's ICAR_CU_* arrays and the column workspace:
 *     36 arrays x (min(kme - kms, 128) + 2) levels x min(nx ny, 32768) columns of REAL(4), and 5 values per column beside it.  hpbl
 *     is filled with 1000 unless the context's boundary layer is ICAR_PBL_YSU at that moment (:180-186).
 * icar_hip_cu_nsas == the call of cu_nsas (:363-417) alone on its..ite, jts..jte and the levels kts..kte-1 of icar_hip_step_configure
 *     (kms..kme-1 without one), with itimestep = STEPCU = 1, mp_physics = 5 (ncloud = 2), pgcon absent (0.55) and the driver's
 *     constants: from TEMPERATURE (as diagnostic_update left it), WATER_VAPOR, CLOUD_WATER, CLOUD_ICE, EXNER, DENSITY, W_REAL (W0AVG
 *     without the stochastic term), DZ_INTERFACE, PRESSURE, PRESSURE_INTERFACE, U_MASS, V_MASS (they set the downdraft's edt),
 *     SENSIBLE_HEAT, LATENT_HEAT (qfx = latent_heat / 2260000), LAND_MASK (never uploaded = all land; XLAND = 2 where the mask is 0 or
 *     2) and hpbl -- ICAR_YSU_HPBL once YSU is initialised (pbl precedes convect in the sub-step), ICAR_NSAS_HPBL otherwise --
 *     -> ICAR_CU_TEND_TH, ICAR_CU_TEND_QV, ICAR_NSAS_TEND_QC, ICAR_NSAS_TEND_QI, ICAR_CU_RAINCV (the deep and the shallow rain),
 *     ICAR_NSAS_PRATEC, ICAR_NSAS_HBOT, ICAR_NSAS_HTOP of those columns; nothing else is touched.  Bit-identical to the compiled
 *     reference.  nsas2d's kbmax, kbm and kmax are made per row from ALL columns its..ite of the row (cu_nsas.f90:619-632): over
 *     terrain a column's result depends on which columns share its row and tile, so an N-image run may differ from the one-image run,
 *     in the reference and here.  tend%u / tend%v are not built: convect applies neither (:502-507 is commented out), and nothing
 *     evaluated reads the updated winds (icar_amd/csrc/nsas_column.h has the derivation).  Levels: kts = 1, at least 3 levels
 *     kts..kte (with one scheme level the reference reads xlamue(i,0), cu_nsas.f90:2456), at most 129; all refused before any launch.
 * icar_hip_convect / _substep / _step / _step_n run this scheme when icar_hip_convection_init selected it: the four tendencies and
 *     RAINCV are zeroed, the scheme runs, the four are applied with their fractions and RAINCV is added to the two precipitation
 *     sums; the whole of diagnostic_update, w_real included, precedes convect in the sub-step.
 * icar_hip_nsas_upload / _download: the scheme's own arrays by ICAR_NSAS_*, REAL(4): the two tendencies (nx,nz,ny), the rest (nx,ny).
 *     hpbl is a restart variable and may be uploaded. */
enum { ICAR_CU_NSAS = 4 };
enum icar_hip_nsas_array {
    ICAR_NSAS_TEND_QC = 0,         /* domain%tend%qc (nx,nz,ny)                                                   */
    ICAR_NSAS_TEND_QI = 1,         /* domain%tend%qi (nx,nz,ny)                                                   */
    ICAR_NSAS_PRATEC = 2,          /* cu_driver.f90's PRATEC of the last call (mm/s)                              */
    ICAR_NSAS_HBOT = 3,            /* lowest_convection_layer, highest_convection_layer of the last call          */
    ICAR_NSAS_HTOP = 4,            /*   (level indices as REAL(4); kte and 0 without convection)                  */
    ICAR_NSAS_HPBL = 5,            /* domain%hpbl%data_2d as init_convection left it (read while YSU is not initialised) */
    ICAR_NSAS_N = 6
};
int icar_hip_convection_init(icar_hip_ctx *ctx, int convection, float stochastic_cu, float tendency_fraction, float tend_qv_fraction,
                             float tend_qc_fraction, float tend_th_fraction, float tend_qi_fraction, const float *znu, float dx);
int icar_hip_cu_nsas(icar_hip_ctx *ctx, float dt, int its, int ite, int jts, int jte);
int icar_hip_nsas_upload(icar_hip_ctx *ctx, int which, const void *host);
int icar_hip_nsas_download(icar_hip_ctx *ctx, int which, void *host);

/* ---- T2: CFL reduction for compute_dt (src/main/time_step.f90:217-330, cfl_strictness 3) -----
 * out = max over the tile of max(|u_i|,|u_i+1|)/dx + max(|v_j|,|v_j+1|)/dx + max(|w_k|,|w_k-1|)/dz_levels(k).
 * A NaN among the winds a cell reads makes the result NaN (the reference's MAX would drop it and step on with a dt of the other
 * cells): icar_hip_compute_dt / _update_dt / _step / _step_n then fail with "the CFL maximum is NaN (the winds contain NaN)". */
int icar_hip_max_courant(icar_hip_ctx *ctx, float dx, const float *dz_levels, float *out);
/* Same reduction, result left in DEVICE memory at d_out (one REAL(4) owned by the caller), no host synchronisation:
 * `call co_min(seconds)` (time_step.f90:413) becomes a 1-element all-reduce(max) of d_out over the images on the device
 * (dt = cfl_reduction_factor / max is monotone, so the minimum dt is the quotient of the maximum). */
int icar_hip_max_courant_device(icar_hip_ctx *ctx, float dx, const float *dz_levels, void *d_out);
/* the same reduction taken ahead of time, on the current stream (typically the second one, beside the advection, right after the
 * forcing of u, v, w): the next icar_hip_max_courant / _device call with the same arguments returns this value without launching
 * anything, provided no entry point has written u, v or w in between (the library counts those writes; handing out a raw
 * device pointer to a wind field disables the shortcut for good). */
int icar_hip_max_courant_prefetch(icar_hip_ctx *ctx, float dx, const float *dz_levels);
/* the other cfl_strictness settings (:238-259, :293-305) also need out[0..2] = maxval(abs(u)), maxval(abs(v)), maxval(abs(w)) */
int icar_hip_max_abs_winds(icar_hip_ctx *ctx, float out[3]);

/* ---- T3: diagnostic_update (src/main/time_step.f90:49-198) ------------------------------------
 * exner=(p/1e5)^(Rd/cp), interface pressure/temperature, surface pressure, T=theta*exner,
 * rho=p/(Rd T), u_mass, v_mass, w_real (uses DZDX, DZDY, JACOBIAN).  The optional column integrals ivt / iwv / iwl / iwi
 * (compute_ivt, compute_iq: src/utilities/atm_utilities.f90:35-102) are computed for every one of ICAR_F_IVT..IWI the
 * host has uploaded once (= `associated(domain%ivt%data_2d)`); iwl / iwi sum the hydrometeor fields that are on the
 * device, like the reference's `associated` tests.  The 10 m winds and ustar (:143-161) likewise once ICAR_F_ROUGHNESS_Z0 has
 * been uploaded (icar_hip_diag_10m). */
int icar_hip_diagnostic_update(icar_hip_ctx *ctx);
/* the same in two parts, for a host that overlaps: parts = 1: everything but w_real (what the microphysics and the advection
 * read: exner, density ...) ; 2: w_real only (:165-194; read by WSM3 and the output, not by Thompson / mp_simple / WSM6 / advect:
 * a streaming kernel that can run beside the VALU-bound interior microphysics) ; 3: both = icar_hip_diagnostic_update. */
int icar_hip_diagnostic_update_parts(icar_hip_ctx *ctx, int parts);

/* ---- F1: apply_forcing / enforce_limits (src/objects/domain_obj.f90:2383-2448, 2228-2243) ----
 * dqdt mirrors variable_t%dqdt_3d.  For each listed field: force_boundaries[i]!=0 -> only the true
 * domain edges named by the west/east/south/north flags (W/E columns without corners, S/N full
 * rows) get  x += dqdt*dt ; otherwise the whole field does (u, v, w, pressure ...).  dt is REAL(8)
 * like time_delta_t%seconds(). */
int icar_hip_dqdt_upload(icar_hip_ctx *ctx, int field, const void *host);
int icar_hip_dqdt_download(icar_hip_ctx *ctx, int field, void *host);
int icar_hip_apply_forcing(icar_hip_ctx *ctx, double dt_seconds, const int *fields, const int *force_boundaries, int nfields,
                           int west_boundary, int east_boundary, int south_boundary, int north_boundary);
int icar_hip_enforce_limits(icar_hip_ctx *ctx, const int *fields, int nfields);

/* ---- W1: balance_uvw (src/physics/wind.f90:81-169): w from the horizontal divergence ---------- */
int icar_hip_balance_uvw(icar_hip_ctx *ctx, float dx);
/* same on u/v/w%meta_data%dqdt_3d -- the form update_winds uses at every forcing step after the first
 * (src/physics/wind.f90:341-360); the w tendency mirror is created if needed. */
int icar_hip_balance_uvw_update(icar_hip_ctx *ctx, float dx);

/* ---- make_winds_grid_relative (src/physics/wind.f90:236-287): rotate the forcing winds from E-W / N-S to the grid's
 * orientation -- destagger u, v to the mass grid, rotate by ICAR_F_SINTHETA / ICAR_F_COSTHETA (REAL(8), (nx,ny)),
 * restagger, extrapolate the two lost edge cells.  update_winds calls it on both of its branches (:300 on u, v; :338 on
 * their dqdt_3d when update != 0).  Not the identity even for an unrotated grid (the double averaging smooths). */
int icar_hip_make_winds_grid_relative(icar_hip_ctx *ctx, int update);

/* ---- iterative_winds (src/physics/wind.f90:371-498), SURVEY 8(f) rank 4 -----------------------
 * The host keeps the reference's control flow: [exchange_u, exchange_v], balance_uvw, correct_w, then
 * wind_iterations+1 times { sweep(1); exchange_u; exchange_v }.  On one image the exchanges are no-ops and
 * sweep(wind_iterations+1) runs the whole loop.  update != 0 works on u/v/w%meta_data%dqdt_3d (wind.f90:392-401).
 *   correct_w  :430-441  w(i,k,j) -= min(sum(dz(1:k))/sum(dz), 1) * w(i,kme,j)
 *   sweep      :455-481  div = calc_divergence(u,v,w) (:172-228); ADJ = div/(-2/dx); u, v faces +-ADJ*0.5 */
int icar_hip_iterative_winds_correct_w(icar_hip_ctx *ctx, int update);
int icar_hip_iterative_winds_sweep(icar_hip_ctx *ctx, float dx, int nsweeps, int update);

/* mass_conservative_acceleration (src/physics/wind.f90:500-511): u = u / ICAR_F_ZR_U, v = v / ICAR_F_ZR_V on the winds
 * (update == 0) or on their meta_data%dqdt_3d (update != 0), as update_winds does for windtype kCONSERVE_MASS */
int icar_hip_mass_conservative_acceleration(icar_hip_ctx *ctx, int update);

/* ---- update_winds (src/physics/wind.f90:289-369) in ONE call ------------------------------------
 * make_winds_grid_relative -> [linear_perturb (windtype 1, 5)] -> [mass_conservative_acceleration (2)] ->
 * [iterative_winds (3, 5): exchange_u / exchange_v, balance_uvw, correct_w, wind_iterations+1 x { sweep; exchange_u;
 * exchange_v } (:371-498)] -> balance_uvw, on u, v, w (update = 0: the first call of a run) or on their
 * meta_data%dqdt_3d (update = 1: every later forcing step); update < 0 lets the context decide like the reference's
 * `if (.not.allocated(domain%sintheta))`.  The staggered exchanges use the context's communicator (icar_hip_comm_init /
 * _init_host), so a multi-image host gets the same winds as a single-image one on the cells it owns.  dx = domain%dx,
 * halo = grid%halo_size, wind_iterations = options%parameters%wind_iterations.  Needs what the parts need: SINTHETA /
 * COSTHETA uploaded (init_winds, :512-590), the linear-wind LUT built for windtype 1 / 5, ZR_U / ZR_V for 2. */
int icar_hip_update_winds(icar_hip_ctx *ctx, int windtype, int wind_iterations, float dx, int halo, int update);
/* `call domain%u%exchange_u(); call domain%v%exchange_v()` (src/objects/exchangeable_obj.f90:158-229) on u, v
 * (update = 0) or their dqdt_3d (1): one message per neighbour through the context's communicator.  Collective. */
int icar_hip_exchange_uv(icar_hip_ctx *ctx, int halo, int update);

/* ---- W3: linear-theory wind look-up table (src/physics/linear_winds.f90) ----------------------
 * options%lt_options (src/objects/options_obj.f90:1400-1530; defaults there: buffer 50, stability_window_size 10,
 * vert_smooth 10, max/min_stability 6e-4/1e-7, N_squared 3e-5, linear_contribution 1, linear_update_fraction 0.2,
 * dir 0..2pi x24, spd 0..30 x6, nsq log(min)..log(max) x5, minimum_layer_size 100). */
typedef struct icar_hip_lt_options {
    int buffer, stability_window_size, vert_smooth;
    int variable_N, smooth_nsq;
    float max_stability, min_stability, N_squared, linear_contribution, linear_update_fraction;
    float dirmax, dirmin, spdmax, spdmin, nsqmax, nsqmin;
    int n_dir_values, n_nsq_values, n_spd_values;
    float minimum_layer_size;
} icar_hip_lt_options;

/* setup_linwinds (:1180-1225): buffered + edge-blended + smoothed terrain (add_buffer_topo :351-418, twice),
 * forward 2-D FFT / (nx*ny), fftshift (single-precision temp, src/utilities/fftshift.f90:95-117), the wavenumber
 * axes of initialize_linear_theory_data (:426-470), the LUT axes (:648-650) and zeroed hi_[uv]_perturbation.
 * global_terrain is domain%global_terrain (nx_global, ny_global) Fortran order; ids/jds = global index of its first
 * cell in the index space of the context's ims/jms (1 in the reference). */
int icar_hip_linwinds_setup(icar_hip_ctx *ctx, const icar_hip_lt_options *opt, const float *global_terrain,
                            int nx_global, int ny_global, int ids, int jds, float dx);
/* domain%terrain_frequency as (re,im) pairs, (fftnx, fftny) Fortran order; out may be NULL to query the size. */
int icar_hip_linwinds_terrain_frequency(icar_hip_ctx *ctx, double *out, size_t capacity_complex, int *fftnx, int *fftny);
/* linear_perturbation (constant-z form, :239-276 -> linear_perturbation_at_height :181-237): real parts of
 * lt_data%u_perturb / v_perturb on the (fftnx, fftny) grid, host buffers. */
int icar_hip_linear_perturbation(icar_hip_ctx *ctx, float U, float V, float Nsq, float z_bottom, float z_top,
                                 float minimum_step, double *u_perturb, double *v_perturb);
/* initialize_spatial_winds (:596-830), constant-z branch: every (dir, spd, N^2) x level entry for this context's
 * tile; z_bottom/z_top[nz] = layer_height -/+ dz_levels/2 (:751-753). */
int icar_hip_linwinds_build_lut(icar_hip_ctx *ctx, const float *z_bottom, const float *z_top, int nz);
/* same, options%parameters%space_varying_dz branch (:738-748 -> linear_perturbation_varyingz :280-344):
 * z_bottom = global_z_interface - global_terrain, z_top = z_bottom + global_dz_interface, both
 * (nx_global, nz, ny_global) Fortran order. */
int icar_hip_linwinds_build_lut_varying(icar_hip_ctx *ctx, const float *z_bottom, const float *z_top, int nz);
/* hi_u_LUT / hi_v_LUT in the reference's index order (n_spd, n_dir, n_nsq, nx[+1], nz, ny[+1]) -- the order of the
 * disk cache src/io/lt_lut_io.f90 -- component 0 = u, 1 = v.  upload replaces read_LUT (:659). */
int icar_hip_linwinds_lut_download(icar_hip_ctx *ctx, int component, float *host);
int icar_hip_linwinds_lut_upload(icar_hip_ctx *ctx, int component, const float *host);
/* one entry hi_u_LUT(spd, dir, nsq, :, :, :) / hi_v_LUT(...) (0-based indices) as a field of the tile's u / v shape (Fortran
 * order (nx[+1], nz, ny[+1])): a production LUT is tens of GB, an entry 20-40 MB */
int icar_hip_linwinds_lut_entry(icar_hip_ctx *ctx, int component, int spd, int dir, int nsq, float *host);
/* hi_u_perturbation / hi_v_perturbation (the relaxed perturbation state, :1263-1268), for restarts and tests. */
int icar_hip_linwinds_perturbation_download(icar_hip_ctx *ctx, int component, float *host);
int icar_hip_linwinds_perturbation_upload(icar_hip_ctx *ctx, int component, const float *host);

/* ---- W2: spatial_winds (:840-1127, reverse=.false.) -------------------------------------------
 * N^2 (calc_stability, src/utilities/atm_utilities.f90:401-467) -> clamp -> log -> vertical (+-vert_smooth) and
 * horizontal (smooth_array ydim=3, src/utilities/array_utilities.f90:308-417) smoothing -> per cell bracket search
 * and 8-corner interpolation of the LUTs -> relaxation of hi_[uv]_perturbation -> added to U/V (update=0) or to their
 * dqdt_3d mirrors (update=1).  Reads POTENTIAL_TEMPERATURE, EXNER, Z, WATER_VAPOR and whichever of CLOUD_WATER,
 * CLOUD_ICE, RAIN, SNOW are on the device ("associated"); writes NSQUARED. */
int icar_hip_spatial_winds(icar_hip_ctx *ctx, int update);

/* ---- F2: the forcing update of the outer loop (src/main/driver.f90:133-137) ---------------------------------------------------------
 * After boundary%update_forcing (the NetCDF read, which stays with the host) the host uploads the small low-resolution arrays it has
 * just read and the device turns them into dqdt_3d rates; nothing of the model state crosses the bus.
 * icar_hip_forcing_configure: the look-up tables the reference builds at init time (geo_LUT, src/utilities/geo_reader.f90:903-976; vLUT,
 *     src/utilities/vinterp.f90:101-152) for forcing%geo (mass grid: nx, ny the context's tile), forcing%geo_u and %geo_v (the EXTENDED
 *     staggered grids u_grid2d_ext / v_grid2d_ext, src/objects/domain_obj.f90:2177-2182; i0, j0 = u_grid%ims - u_grid2d_ext%ims and
 *     u_grid%jms - u_grid2d_ext%jms, likewise for v; both NULL: u and v cannot be forced), domain%nsmooth, and forcing%geo%z (nx, nz_f, ny)
 *     with domain%geo%z (nx, nz, ny) for adjust_pressure (both NULL: the pressure cannot be forced).  Arrays in Fortran element order, as
 *     the reference holds them: x, y, w (4, nx, ny); z, zw (2, nx, nz, ny), nz the context's.  EVERY index is checked on the host before
 *     anything is stored -- x in 1..nx_f, y in 1..ny_f, z in 1..nz_f, the mass tables' extents against the context, the tile inside the
 *     extended grid, nsmooth within 1..the extended grid's width (smooth_array reads rowmeans(2:windowsize)), and nz_f >= nz when
 *     forcing%geo%z is given (adjust_pressure indexes it with the model's nz; the reference reads out of bounds otherwise) -- and a bad
 *     table is refused with a message that names the array and the element.  time_varying_z != 0 is refused: not built.
 * icar_hip_forcing_upload: input_data%data_3d of the forcing variable of `field`, (nx_f, nz_f, ny_f), as just read.  _download reads
 *     it back (tests: interpolate_variable smooths the forcing's own u / v IN PLACE, :2775, :2798, and so does the device copy).
 * icar_hip_interpolate_forcing == domain%interpolate_forcing(forcing, update) (domain_obj.f90:2559-2643) over the listed 3-D fields
 *     (variables_to_force): update != 0 writes their dqdt_3d mirrors (created if needed), update == 0 the fields themselves
 *     (get_initial_conditions).  Mass-grid fields: geo_interp (geo_reader.f90:1069-1136) and vinterp (vinterp.f90:284-295), fused, all of
 *     them in one launch.  ICAR_F_U / ICAR_F_V: smooth_array(input, 1) on the forcing's array in place, geo_interp onto the extended
 *     grid, vinterp, smooth_array(.., nsmooth), the tile's sub-box (:2764-2806).  pressure_field (-1: none): no vertical interpolation
 *     (:2750-2760), then adjust_pressure (:2656-2702, update_pressure src/utilities/atm_utilities.f90:611-653) with the forcing data of
 *     theta_field likewise not interpolated vertically.  Bit-identical to the compiled reference.  Refused before any launch: a call
 *     before forcing_configure, a 2-D field (geo_interp2d is not built), a field without forcing data or with data of other extents
 *     than its tables, u / v or the pressure without their tables.
 * icar_hip_update_delta_fields == domain%update_delta_fields(dt) (:2339-2372): dqdt_3d = (dqdt_3d - data_3d) / dt%seconds() for the
 *     listed fields and for ICAR_F_W, always (:2368-2369); the difference in REAL(4), the quotient in REAL(8) as dt%seconds() is
 *     (src/utilities/time_delta_obj.f90:123-130), rounded once.
 * icar_hip_forcing_step == driver.f90:133-137 in one call: interpolate_forcing(update = 1), icar_hip_update_winds(.., update = 1),
 *     update_delta_fields; the same bits as the three calls made one after the other. */
typedef struct icar_hip_forcing_geo {
    const int *x, *y;              /* geolut%x, %y  INTEGER (4, nx, ny): 1-based indices into the forcing grid       */
    const float *w;                /* geolut%w      REAL    (4, nx, ny); w(4) is never read                          */
    const int *z;                  /* vert_lut%z    INTEGER (2, nx, nz, ny): 1-based forcing levels                   */
    const float *zw;               /* vert_lut%w    REAL    (2, nx, nz, ny)                                          */
    int nx, ny;                    /* the tables' grid: the tile (mass) or the extended staggered grid (u, v)        */
    int nx_f, nz_f, ny_f;          /* extents of the forcing arrays these tables index                               */
    int i0, j0;                    /* u, v: 0-based offset of the tile's staggered grid in the extended grid         */
} icar_hip_forcing_geo;
int icar_hip_forcing_configure(icar_hip_ctx *ctx, const icar_hip_forcing_geo *mass, const icar_hip_forcing_geo *u, const icar_hip_forcing_geo *v,
                               int nsmooth, const float *forcing_z, const float *domain_z, int time_varying_z);
int icar_hip_forcing_upload(icar_hip_ctx *ctx, int field, const float *lo, int nx_f, int nz_f, int ny_f);
int icar_hip_forcing_download(icar_hip_ctx *ctx, int field, float *lo, size_t count);
int icar_hip_interpolate_forcing(icar_hip_ctx *ctx, const int *fields, int nfields, int pressure_field, int theta_field, int update);
int icar_hip_update_delta_fields(icar_hip_ctx *ctx, const int *fields, int nfields, double dt_seconds);
int icar_hip_forcing_step(icar_hip_ctx *ctx, const int *fields, int nfields, int pressure_field, int theta_field, int windtype,
                          int wind_iterations, float dx, int halo, double dt_seconds);

/* ---- F3: the 2-D forced variables (variables_to_force, src/objects/domain_obj.f90:199, :212, :215, :272) -----------------------------
 * sst, shortwave, longwave and external_precipitation through the same three places as the 3-D ones.  data_2d of the first three is the
 * field slot (ICAR_F_SST, ICAR_F_SHORTWAVE, ICAR_F_LONGWAVE); external_precipitation%data_2d has no slot and is owned by the forcing
 * state.  A context that never calls these issues exactly what it issued before; the 3-D entry points above keep refusing 2-D fields.
 * All of them need icar_hip_forcing_configure first (the mass grid's geolut is the one geo_interp2d reads), _get / _set excepted.
 * icar_hip_forcing2d_upload: input_data%data_2d (nx_f, ny_f) of the forcing variable as just read; the extents must be those of the
 *     mass tables given to icar_hip_forcing_configure.  _download reads it back.
 * icar_hip_interpolate_forcing_2d == the two_d branch of domain%interpolate_forcing (domain_obj.f90:2595-2600): geo_interp2d
 *     (src/utilities/geo_reader.f90:1142-1182) over the whole memory ims:ime, jms:jme, all listed variables in one launch; update != 0
 *     writes dqdt_2d (created if needed), update == 0 data_2d.
 * icar_hip_update_delta_fields_2d == domain_obj.f90:2355-2356: dqdt_2d = (dqdt_2d - data_2d) / dt%seconds(), the difference in REAL(4),
 *     the quotient in REAL(8), rounded once.
 * icar_hip_apply_forcing_2d == domain_obj.f90:2400-2402 for the enabled set, data_2d = data_2d + (dqdt_2d * dt%seconds()) in REAL(8)
 *     rounded once, and :2438-2445: accumulated_precipitation%data_2dd (ICAR_F_PRECIPITATION) takes external_precipitation * dt.  One
 *     launch.  As the reference's `associated` tests do, it passes over an enabled variable whose data_2d or dqdt_2d is not on the device
 *     and over the sum while ICAR_F_PRECIPITATION is not on the device (or external_precipitation is not enabled): neither is an error.
 * icar_hip_forcing2d_enable: the variables icar_hip_forcing_step also interpolates (update) and takes the delta of, and that
 *     icar_hip_substep / _step / _step_n apply at src/main/time_step.f90:534 on the main stream behind the 3-D forcing with the
 *     sub-step's own dt.  n = 0 disables.
 * icar_hip_forcing2d_get / _set: data_2d (ICAR_FORCED2D_DATA) or dqdt_2d (ICAR_FORCED2D_DQDT) of one variable, (nx, ny) REAL(4): for a
 *     restart and for tests (external_precipitation has no field slot to go through).  _set creates the array.
 * Refused before any launch, with a text that names the cause and the state left as it was: a call before forcing_configure, a bad id, a
 * variable listed twice, a variable without uploaded data, data of other extents than the tables, dt not a positive finite number, a
 * delta for a variable that has no dqdt_2d (or no data_2d).  Bit-identical to the compiled reference. */
typedef enum icar_hip_forced2d {
    ICAR_FORCED2D_SST = 0,                     /* domain%sst                      data_2d = ICAR_F_SST       */
    ICAR_FORCED2D_SHORTWAVE = 1,               /* domain%shortwave                data_2d = ICAR_F_SHORTWAVE */
    ICAR_FORCED2D_LONGWAVE = 2,                /* domain%longwave                 data_2d = ICAR_F_LONGWAVE  */
    ICAR_FORCED2D_EXTERNAL_PRECIPITATION = 3,  /* domain%external_precipitation   owned by the forcing state */
    ICAR_FORCED2D_N = 4
} icar_hip_forced2d;
enum { ICAR_FORCED2D_DATA = 0, ICAR_FORCED2D_DQDT = 1 };
int icar_hip_forcing2d_upload(icar_hip_ctx *ctx, int which, const float *lo, int nx_f, int ny_f);
int icar_hip_forcing2d_download(icar_hip_ctx *ctx, int which, float *lo, size_t count);
int icar_hip_interpolate_forcing_2d(icar_hip_ctx *ctx, const int *which, int n, int update);
int icar_hip_update_delta_fields_2d(icar_hip_ctx *ctx, const int *which, int n, double dt_seconds);
int icar_hip_apply_forcing_2d(icar_hip_ctx *ctx, double dt_seconds);
int icar_hip_forcing2d_enable(icar_hip_ctx *ctx, const int *which, int n);
int icar_hip_forcing2d_get(icar_hip_ctx *ctx, int which, int what, float *host);
int icar_hip_forcing2d_set(icar_hip_ctx *ctx, int which, int what, const float *host);

/* ---- H1: halo faces (src/objects/exchangeable_obj.f90:138-356) --------------------------------
 * dir: 0=north 1=south 2=east 3=west.  pack gathers what exchangeable%put_<dir> would PUT
 * (my interior planes next to that edge, width halo, N/S over the full memory width so corners
 * travel) for all listed fields into one contiguous device buffer; unpack scatters a received
 * buffer into my halo planes like retrieve_<dir>_halo.  Buffers are device pointers; the element
 * count per field is icar_hip_halo_count(). */
size_t icar_hip_halo_count(const icar_hip_ctx *ctx, int dir, int halo);
/* Staggered faces: exchange_u / exchange_v (exchangeable_obj.f90:158-229) move halo+1 planes in the staggered
 * direction, which the cell-grid packers above cannot express.  box_pack gathers the 0-based box
 * [i0, i0+ni) x all levels x [j0, j0+nj) of one REAL(4) 3-D field (which = 0: data_3d, 1: meta_data%dqdt_3d) into a
 * device buffer laid out [nj][nz][ni]; box_unpack scatters it back.  icar_amd/halo.py holds the index table. */
int icar_hip_box_pack(icar_hip_ctx *ctx, int field, int which, int i0, int ni, int j0, int nj, void *dbuf);
int icar_hip_box_unpack(icar_hip_ctx *ctx, int field, int which, int i0, int ni, int j0, int nj, const void *dbuf);
int icar_hip_halo_pack(icar_hip_ctx *ctx, int dir, int halo, const int *fields, int nfields, void *dbuf);
int icar_hip_halo_unpack(icar_hip_ctx *ctx, int dir, int halo, const int *fields, int nfields, const void *dbuf);
/* the same for several directions in ONE launch (dirs[z], dbufs[z], z < ndirs <= 4): what domain%halo_send /
 * halo_retrieve (objects/domain_obj.f90:109-143) issue per step -- 2 launches instead of 8 for an image with 4 neighbours */
int icar_hip_halo_pack_dirs(icar_hip_ctx *ctx, int ndirs, const int *dirs, int halo, const int *fields, int nfields, void *const *dbufs);
int icar_hip_halo_unpack_dirs(icar_hip_ctx *ctx, int ndirs, const int *dirs, int halo, const int *fields, int nfields, void *const *dbufs);

/* ---- H1 transport + co_min: domain%halo_send / halo_retrieve (src/objects/domain_obj.f90:109-143 over
 * src/objects/exchangeable_obj.f90:138-356) and `call co_min(seconds)` (src/main/time_step.f90:413) -------------------
 * One message per neighbour carries every exchanged scalar (the reference PUTs once per variable and direction).
 * neighbors[dir] (dir 0=north 1=south 2=east 3=west) is the 0-based rank of the image on that side (= image - 1 of
 * grid_t's neighbour), ICAR_NEIGHBOR_NONE at a domain boundary, or ICAR_NEIGHBOR_SELF for an edge that wraps around to the
 * tile's own opposite edge (periodic single image, what src/tests/test_mpdata.f90 does by hand; both edges of an axis).
 *   icar_hip_comm_init       RCCL (ncclSend / ncclRecv over xGMI on the context's stream, nothing waits on the host).
 *                            uid = the 128 bytes image 1 got from icar_hip_comm_unique_id and broadcast (co_broadcast in a
 *                            coarray host); uid == NULL is allowed for one image without peers.
 *                            One GPU per image: RCCL refuses two ranks on one device.
 *   icar_hip_comm_init_host  the same entry points with the messages staged through POSIX shared memory `shm_name`
 *                            (unique per run; slot_bytes >= the largest message = max halo_count * number of exchanged
 *                            fields * 4, the same on every image): for boxes with fewer GPUs than images.  A functional
 *                            path, not a fast one.
 * halo_send packs (one launch) and posts the transfers; halo_retrieve is the `sync images` + unpack (one launch, the
 * reference's N, S, E, W precedence at the corner cells).  Exactly one halo_retrieve per halo_send, same arguments. */
enum { ICAR_NEIGHBOR_NONE = -1, ICAR_NEIGHBOR_SELF = -2 };
enum { ICAR_COMM_NONE = 0, ICAR_COMM_LOCAL = 1, ICAR_COMM_RCCL = 2, ICAR_COMM_HOST = 3 };
int icar_hip_comm_unique_id(char uid[128]);
int icar_hip_comm_init(icar_hip_ctx *ctx, int nranks, int rank, const char uid[128], const int neighbors[4]);
int icar_hip_comm_init_host(icar_hip_ctx *ctx, int nranks, int rank, const char *shm_name, size_t slot_bytes, const int neighbors[4]);
int icar_hip_comm_destroy(icar_hip_ctx *ctx);
int icar_hip_comm_kind(icar_hip_ctx *ctx);                      /* ICAR_COMM_* */
/* how long the host-staged transport waits for a neighbouring image before it reports an error (default 60 s; a debugger or
 * a long host pause on a neighbour wants more).  Process-wide. */
int icar_hip_comm_timeout(double seconds);
/* num_images() as the transport itself reports it (ncclCommCount / the shared segment's header; 1 without a transport) */
int icar_hip_comm_ranks(icar_hip_ctx *ctx, int *nranks);
/* A self-test of exchangeable_t%send / %retrieve (src/objects/exchangeable_obj.f90:138-356) on this communicator: one
 * exchange of a field stamped with this image's number, verified on the device -- every halo cell must carry the stamp of
 * the neighbour on its side (corner cells aside).  The field used (water vapour) is restored.  n_bad = offending cells.
 * Collective: every image of the communicator calls it. */
int icar_hip_halo_selfcheck(icar_hip_ctx *ctx, int halo, int *n_bad);
int icar_hip_halo_send(icar_hip_ctx *ctx, int halo, const int *fields, int nfields);
int icar_hip_halo_retrieve(icar_hip_ctx *ctx, int halo, const int *fields, int nfields);
/* in/out: *value becomes the minimum (maximum) over the images; one image: unchanged */
int icar_hip_co_min(icar_hip_ctx *ctx, double *value);
int icar_hip_co_max(icar_hip_ctx *ctx, double *value);

/* ---- T1 / T2 / M0: the sub-step loop itself (src/main/time_step.f90:440-551) ----------------------------------------
 * icar_hip_step_configure hands the library the members of options_t / grid_t the loop reads; after that
 *   icar_hip_compute_dt  == compute_dt (:217-330) on this image's tile
 *   icar_hip_update_dt   == update_dt (:375-423): compute_dt (:217-330, every cfl_strictness) + co_min + the 120 s cap;
 *                           fails with "ERROR time step too small" where the reference stops (:322-328)
 *   icar_hip_mp          == mp(domain, options, dt, halo, subset) (src/physics/mp_driver.f90:673-772) incl. the
 *                           update_interval gating (:698-713); halo / subset < 0 = argument not present
 *   icar_hip_advect_step == advect(domain, options, dt) (src/physics/advection_driver.f90:51-77)
 *   icar_hip_substep     == one pass of :474-539: diagnostic_update -> [rad -> lsm -> pbl -> convect, each when configured] -> mp(halo=1) -> halo_send -> mp(subset=1) ->
 *                           halo_retrieve -> advect -> apply_forcing [-> enforce_limits], with the interior microphysics and
 *                           the streaming kernels issued on the context's second stream beside the heavy ones
 *   icar_hip_step        == step(domain, end_time, options) (:440-551); the model clock lives in the context.
 *                           An error from icar_hip_step / icar_hip_step_n leaves the fields undefined (the reference STOPs
 *                           where update_dt fails, :322-328): when the failing sub-step had already been opened the context
 *                           is marked failed and every stepping entry point returns an error until the caller has reloaded
 *                           the fields and set the clock again (icar_hip_model_time_set).  Clearing the mark is a restart:
 *                           icar_hip_model_time_set then also puts last_model_time of the microphysics back to -999, as
 *                           icar_hip_mp_reset does, so that the next microphysics call is a first one (mp_dt = max(update_interval,
 *                           dt)) and the context continues as a newly created one with the same fields and clock would.  On a
 *                           context that is not marked failed icar_hip_model_time_set sets the clock and nothing else.  When
 *                           update_dt fails with no sub-step opened the context is not marked: its fields and clock are those
 *                           after the last completed sub-step (diagnostics aside, see below), and stepping may go on.
 *                           The DIAGNOSTIC fields (temperature, density, pressure_interface, surface_pressure,
 *                           temperature_interface, u_mass, v_mass, w_real) after icar_hip_step / icar_hip_step_n are those of
 *                           the call's LAST sub-step -- what the reference leaves, too; the sub-steps before it write only the
 *                           diagnostics that something on the device reads (exner always), since the host cannot look between
 *                           them.  They are unspecified if the call fails part-way.  icar_hip_substep is its own last sub-step.
 * The library keeps the model clock (domain%model_time) and mp_driver.f90's SAVE variable last_model_time. */
typedef struct icar_hip_step_config {
    int advection;                  /* options%physics%advection: 0, ICAR_ADV_UPWIND, ICAR_ADV_MPDATA            */
    int microphysics;               /* options%physics%microphysics: 0, 1 Thompson, 2 mp_simple, 4 WSM6, 6 WSM3  */
    int mpdata_order;               /* options%adv_options%mpdata_order                                           */
    int flux_corrected_transport;   /* options%adv_options%flux_corrected_transport                               */
    int advect_density;             /* options%parameters%advect_density                                          */
    int cfl_strictness;             /* options%parameters%cfl_strictness (1..5)                                   */
    float cfl_reduction_factor;     /* options%parameters%cfl_reduction_factor                                    */
    float dx;                       /* domain%dx                                                                  */
    float mp_update_interval;       /* options%mp_options%update_interval                                         */
    int top_mp_level;               /* options%mp_options%top_mp_level                                            */
    int halo_size;                  /* grid%halo_size                                                             */
    int its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde;                     /* grid_t                 */
    int west_boundary, east_boundary, south_boundary, north_boundary;                   /* grid_t                 */
    int diagnostics;                /* 1: diagnostic_update at the top of the sub-step (:474), as the reference   */
    int prefetch_dt;                /* 1: take the CFL reduction of the next update_dt beside the advection       */
    int n_advect, advect_fields[ICAR_N_ADVECTABLE];      /* options%vars_to_advect in the dispatch order of adv_mpdata.f90:512-522 */
    int n_exchange, exchange_fields[ICAR_N_ADVECTABLE];  /* the exchangeable members, halo_send order               */
    int n_forced, forced_fields[16], force_boundaries[16];   /* apply_forcing's variables (domain_obj.f90:2383-2448) */
} icar_hip_step_config;
int icar_hip_step_configure(icar_hip_ctx *ctx, const icar_hip_step_config *cfg, const float *dz_levels);
int icar_hip_model_time_set(icar_hip_ctx *ctx, double seconds);
double icar_hip_model_time(const icar_hip_ctx *ctx);
int icar_hip_mp_reset(icar_hip_ctx *ctx);                       /* mp_init / mp_finish: last_model_time = -999 */
int icar_hip_compute_dt(icar_hip_ctx *ctx, double *dt_seconds);   /* compute_dt alone: this image, no co_min, no cap */
int icar_hip_update_dt(icar_hip_ctx *ctx, double *dt_seconds);
int icar_hip_mp(icar_hip_ctx *ctx, double dt, int halo, int subset);
int icar_hip_advect_step(icar_hip_ctx *ctx, double dt);
int icar_hip_substep(icar_hip_ctx *ctx, double dt_seconds, int enforce_limits);
int icar_hip_step(icar_hip_ctx *ctx, double end_time_seconds, int *nsteps);
/* the same loop for a given NUMBER of sub-steps (update_dt -> substep -> clock += dt each), no end-of-interval clamp and no
 * enforce_limits: what a benchmark times as "K passes of the hot path".  dt_last (may be NULL) receives the last dt.
 * As with icar_hip_step, the diagnostic fields are those of the call's last sub-step (unspecified if the call fails part-way). */
int icar_hip_step_n(icar_hip_ctx *ctx, int nsteps, double *dt_last);

/* ---- measurement helpers --------------------------------------------------------------------- */
/* Average duration (ms) of the launches of a named kernel group since the last reset, measured
 * with HIP events on the context's stream (bench.py roofline block). group: "advect", "mp", "pbl", "rad", "diag_10m", "lsm_water", "lsm_fluxes", "cu_bmj", "cu_stream" ... */
int icar_hip_timing_enable(icar_hip_ctx *ctx, int on);
/* restrict the timers to a comma-separated list of groups ("advect", "advect,mp,winds"; NULL or "" = all): every timed
 * scope costs its stream two timestamped barrier packets, ~5 us -- a dozen groups per sub-step are 10 % of a small tile's step */
int icar_hip_timing_groups(icar_hip_ctx *ctx, const char *groups_csv);
int icar_hip_timing_read(icar_hip_ctx *ctx, const char *group, double *total_ms, int *launches);
int icar_hip_timing_reset(icar_hip_ctx *ctx);

const char *icar_hip_last_error(void);
const char *icar_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ICAR_HIP_H */

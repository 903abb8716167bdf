!> icar_hip_mod.f90 -- Fortran 2008 host side of libicar_hip.so (include/icar_hip.h).
!!
!! `use icar_hip` gives (a) the raw iso_c_binding interfaces of every C-ABI entry point and
!! (b) thin wrappers with the reference's operator names and argument meaning:
!!     call hip_advect(ctx, options%physics%advection, mpdata_order, fct, advect_density, dt, dx, vars)
!!     call hip_mp_simple(ctx, dt, its,ite, jts,jte, kts,kte)
!!     call hip_thompson_init(ctx, mp_options...) ; call hip_thompson(ctx, dt, its..kte, ids..kde)
!! A non-zero return code becomes `error stop` with the library's message -- the reference's own
!! error convention (stop / error stop; SURVEY 8b).  INTEGRATION.md shows where ICAR calls these.
module icar_hip
  use iso_c_binding
  implicit none
  private
  public :: hip_ctx_t, hip_create, hip_destroy, hip_upload, hip_download, hip_upload_2dd, hip_download_2dd, hip_upload_2d, hip_upload_2di, &
            hip_advect, hip_mp_simple, hip_thompson_init, hip_thompson, hip_max_courant, hip_balance_uvw, hip_sync, &
            hip_lt_options_t, hip_setup_linwinds, hip_linwinds_build_lut, hip_spatial_winds, hip_iterative_winds, &
            hip_iterative_winds_correct_w, hip_iterative_winds_sweep, &
            hip_diagnostic_update, hip_diagnostic_update_parts, hip_dqdt_upload, hip_apply_forcing, hip_enforce_limits, hip_halo_count, hip_halo_pack, &
            hip_halo_unpack, hip_mp_simple_tiles, hip_halo_pack_dirs, hip_halo_unpack_dirs, hip_thompson_tiles, hip_mass_conservative_acceleration, hip_balance_uvw_update, hip_wsm3_init, hip_wsm3, hip_wsm6_init, hip_wsm6, hip_wsm6_tiles, hip_winds_valid, hip_max_courant_prefetch, &
            hip_aux_fork, hip_aux_begin, hip_aux_end, hip_aux_join, hip_max_courant_device, hip_make_winds_grid_relative, &
            hip_step_config_t, hip_step_configure, hip_update_dt, hip_compute_dt, hip_substep, hip_step, hip_step_n, hip_mp, hip_advect_step, hip_mp_reset, &
            hip_model_time, hip_set_model_time, hip_comm_unique_id, hip_comm_init, hip_comm_init_local, hip_comm_init_host, hip_comm_destroy, &
            hip_halo_send, hip_halo_retrieve, hip_co_min, hip_comm_ranks, hip_halo_selfcheck, hip_update_winds, hip_exchange_uv, hip_mpdata_exact, &
            hip_pbl_init, hip_ysu_sfc, hip_ysu, hip_ysu_upload, hip_ysu_download, hip_ysu_download_kpbl, ICAR_PBL_YSU, &
            ICAR_YSU_GROUND_SURF_TEMPERATURE, ICAR_YSU_HPBL, ICAR_YSU_KPBL, ICAR_YSU_EXCH_H, ICAR_YSU_PSIM, ICAR_YSU_PSIH, ICAR_YSU_REGIME, ICAR_YSU_RI, &
            ICAR_YSU_WINDSPD, ICAR_YSU_HOL, ICAR_YSU_ZOL, ICAR_YSU_GZ1OZ0, ICAR_YSU_Z_ATM, ICAR_YSU_TEND_TH, ICAR_YSU_TEND_QV, ICAR_YSU_TEND_QC, &
            ICAR_YSU_TEND_QI, ICAR_YSU_TEND_U, ICAR_YSU_TEND_V, ICAR_YSU_N, &
            hip_pbl_configure, hip_pbl, hip_pbl_simple, ICAR_PBL_SIMPLE, hip_rad_configure, hip_rad_calendar, hip_rad, hip_ra_simple, ICAR_RA_SIMPLE, &
            hip_lsm_configure, hip_diag_10m, hip_water_simple, hip_apply_fluxes, hip_lsm, hip_lsm_layers, ICAR_LSM_BASIC, ICAR_WATER_SIMPLE, &
            hip_noah_tables_t, hip_noah_options_t, hip_noah_tables, hip_lsm_init, hip_lsm_noah, hip_noah_upload, hip_noah_upload_int, hip_noah_download, &
            hip_noah_download_int, ICAR_LSM_NOAH, &
            hip_lsm_noah_couple, hip_lsm_upload, hip_lsm_upload_r8, hip_lsm_download, hip_lsm_download_r8, &
            ICAR_LSM_TEMPERATURE_2M, ICAR_LSM_HUMIDITY_2M, ICAR_LSM_LONGWAVE_UP, ICAR_LSM_RAINBL, ICAR_LSM_Z_ATM, ICAR_LSM_LNZ_ATM_TERM, &
            ICAR_LSM_BASE_EXCHANGE_TERM, ICAR_LSM_N, &
            ICAR_NOAH_VEG_TYPE, ICAR_NOAH_SOIL_TYPE, ICAR_NOAH_VEGFRAC, ICAR_NOAH_SOIL_DEEP_TEMPERATURE, ICAR_NOAH_SHDMIN, ICAR_NOAH_SHDMAX, &
            ICAR_NOAH_SNOALB, ICAR_NOAH_QGH, ICAR_NOAH_CHS, ICAR_NOAH_CQS2, ICAR_NOAH_RI, ICAR_NOAH_CURRENT_PRECIPITATION, &
            ICAR_NOAH_GROUND_HEAT_FLUX, ICAR_NOAH_SMSTAV, ICAR_NOAH_SOIL_TOTALMOISTURE, ICAR_NOAH_SFCRUNOFF, ICAR_NOAH_UDRUNOFF, ICAR_NOAH_ALBEDO, &
            ICAR_NOAH_ALBBCK, ICAR_NOAH_Z0, ICAR_NOAH_EMISS, ICAR_NOAH_SNOWC, ICAR_NOAH_SNOW_WATER_EQUIVALENT, ICAR_NOAH_SNOW_HEIGHT, &
            ICAR_NOAH_CANOPY_WATER, ICAR_NOAH_CHS2, ICAR_NOAH_CHKLOWQ, ICAR_NOAH_LAI, ICAR_NOAH_SNOTIME, ICAR_NOAH_ACSNOM, ICAR_NOAH_ACSNOW, &
            ICAR_NOAH_SNOPCX, ICAR_NOAH_POTEVP, ICAR_NOAH_NOAHRES, ICAR_NOAH_FLX4, ICAR_NOAH_FVB, ICAR_NOAH_FBUR, ICAR_NOAH_FGSN, &
            ICAR_NOAH_SOIL_WATER_CONTENT, ICAR_NOAH_SOIL_TEMPERATURE, ICAR_NOAH_SH2O, ICAR_NOAH_SMCREL, ICAR_NOAH_N, &
            hip_cu_configure, hip_cu_bmj, hip_convect, hip_cu_reset, hip_cu_upload, hip_cu_download, ICAR_CU_BMJ, ICAR_CU_NO_STOCHASTIC, &
            hip_cu_init, hip_cu_tiedtke, hip_tiedtke_upload, hip_tiedtke_download, hip_tiedtke_download_ktype, ICAR_CU_TIEDTKE, &
            ICAR_TIEDTKE_TEND_QC, ICAR_TIEDTKE_TEND_QI, ICAR_TIEDTKE_PRATEC, ICAR_TIEDTKE_KTYPE, ICAR_TIEDTKE_N, &
            hip_convection_init, hip_cu_nsas, hip_nsas_upload, hip_nsas_download, ICAR_CU_NSAS, &
            hip_forcing_geo_t, hip_forcing_configure, hip_forcing_upload, hip_interpolate_forcing, hip_update_delta_fields, hip_forcing_step, &
            hip_forcing2d_upload, hip_forcing2d_download, hip_forcing2d_interpolate, hip_forcing2d_update_delta, hip_forcing2d_apply, &
            hip_forcing2d_enable, hip_forcing2d_get, hip_forcing2d_set, ICAR_FORCED2D_SST, ICAR_FORCED2D_SHORTWAVE, ICAR_FORCED2D_LONGWAVE, &
            ICAR_FORCED2D_EXTERNAL_PRECIPITATION, ICAR_FORCED2D_N, ICAR_FORCED2D_DATA, ICAR_FORCED2D_DQDT, &
            ICAR_NSAS_TEND_QC, ICAR_NSAS_TEND_QI, ICAR_NSAS_PRATEC, ICAR_NSAS_HBOT, ICAR_NSAS_HTOP, ICAR_NSAS_HPBL, ICAR_NSAS_N, &
            ICAR_CU_CLDEFI, ICAR_CU_ACC_CONV_PCP, ICAR_CU_RAINCV, ICAR_CU_CUTOP, ICAR_CU_CUBOT, ICAR_CU_TEND_TH, ICAR_CU_TEND_QV, ICAR_CU_N, &
            ICAR_NEIGHBOR_NONE, ICAR_NEIGHBOR_SELF, ICAR_N_ADVECTABLE
  public :: ICAR_F_WATER_VAPOR, ICAR_F_CLOUD_WATER, ICAR_F_RAIN, ICAR_F_SNOW, ICAR_F_POTENTIAL_TEMPERATURE, &
            ICAR_F_CLOUD_ICE, ICAR_F_GRAUPEL, ICAR_F_ICE_NUMBER, ICAR_F_RAIN_NUMBER, ICAR_F_U, ICAR_F_V, ICAR_F_W, &
            ICAR_F_PRESSURE, ICAR_F_EXNER, ICAR_F_DENSITY, ICAR_F_DZ_MASS, ICAR_F_JACOBIAN, ICAR_F_JACOBIAN_U, &
            ICAR_F_JACOBIAN_V, ICAR_F_JACOBIAN_W, ICAR_F_ADVECTION_DZ, ICAR_F_PRECIPITATION, ICAR_F_SNOWFALL, ICAR_F_GRAUPEL_ACC, &
            ICAR_F_Z, ICAR_F_NSQUARED, ICAR_F_PRESSURE_INTERFACE, ICAR_F_TEMPERATURE, ICAR_F_TEMPERATURE_INTERFACE, &
            ICAR_F_U_MASS, ICAR_F_V_MASS, ICAR_F_W_REAL, ICAR_F_DZDX, ICAR_F_DZDY, ICAR_F_SURFACE_PRESSURE, &
            ICAR_F_IVT, ICAR_F_IWV, ICAR_F_IWL, ICAR_F_IWI, ICAR_F_ZR_U, ICAR_F_ZR_V, ICAR_F_SINTHETA, ICAR_F_COSTHETA, &
            ICAR_F_TERRAIN, ICAR_F_LAND_MASK, ICAR_F_LATITUDE, ICAR_F_LONGITUDE, ICAR_F_SHORTWAVE, ICAR_F_LONGWAVE, ICAR_F_CLOUD_FRACTION, &
            ICAR_F_ROUGHNESS_Z0, ICAR_F_U_10M, ICAR_F_V_10M, ICAR_F_USTAR, ICAR_F_SST, ICAR_F_SKIN_TEMPERATURE, ICAR_F_SENSIBLE_HEAT, &
            ICAR_F_LATENT_HEAT, ICAR_F_QSFC, ICAR_F_QFX, ICAR_F_DZ_INTERFACE

  ! struct icar_hip_forcing_geo (include/icar_hip.h) and what a host fills in: pointers to the reference's own look-up tables
  ! (forcing%geo%geolut%x / %y / %w, forcing%geo%vert_lut%z / %w; for u / v those of forcing%geo_u / %geo_v on the extended grids)
  type, bind(C) :: forcing_geo_c
     type(c_ptr) :: x, y, w, z, zw
     integer(c_int) :: nx, ny, nx_f, nz_f, ny_f, i0, j0
  end type
  type hip_forcing_geo_t
     integer(c_int), pointer, contiguous :: x(:,:,:) => null(), y(:,:,:) => null(), z(:,:,:,:) => null()
     real(c_float), pointer, contiguous :: w(:,:,:) => null(), zw(:,:,:,:) => null()
     integer :: nx_f = 0, nz_f = 0, ny_f = 0      ! extents of the forcing variables these tables index
     integer :: i0 = 0, j0 = 0                    ! u, v: u_grid%ims - u_grid2d_ext%ims, u_grid%jms - u_grid2d_ext%jms (likewise v)
  end type

  ! enum icar_hip_field (include/icar_hip.h)
  integer(c_int), parameter :: ICAR_F_WATER_VAPOR=0, ICAR_F_CLOUD_WATER=1, ICAR_F_RAIN=2, ICAR_F_SNOW=3, &
       ICAR_F_POTENTIAL_TEMPERATURE=4, ICAR_F_CLOUD_ICE=5, ICAR_F_GRAUPEL=6, ICAR_F_ICE_NUMBER=7, ICAR_F_RAIN_NUMBER=8, &
       ICAR_F_U=11, ICAR_F_V=12, ICAR_F_W=13, ICAR_F_PRESSURE=14, ICAR_F_EXNER=15, ICAR_F_DENSITY=16, ICAR_F_DZ_MASS=17, &
       ICAR_F_JACOBIAN=18, ICAR_F_JACOBIAN_U=19, ICAR_F_JACOBIAN_V=20, ICAR_F_JACOBIAN_W=21, ICAR_F_ADVECTION_DZ=22, &
       ICAR_F_PRECIPITATION=23, ICAR_F_SNOWFALL=24, ICAR_F_GRAUPEL_ACC=25, ICAR_F_PRESSURE_INTERFACE=26, ICAR_F_TEMPERATURE=27, &
       ICAR_F_TEMPERATURE_INTERFACE=28, ICAR_F_U_MASS=29, ICAR_F_V_MASS=30, ICAR_F_W_REAL=31, ICAR_F_DZDX=32, ICAR_F_DZDY=33, &
       ICAR_F_SURFACE_PRESSURE=34, ICAR_F_Z=35, ICAR_F_NSQUARED=36, ICAR_F_IVT=37, ICAR_F_IWV=38, ICAR_F_IWL=39, ICAR_F_IWI=40, &
       ICAR_F_ZR_U=41, ICAR_F_ZR_V=42, ICAR_F_SINTHETA=43, ICAR_F_COSTHETA=44, ICAR_F_TERRAIN=45, ICAR_F_LAND_MASK=46, &
       ICAR_F_LATITUDE=47, ICAR_F_LONGITUDE=48, ICAR_F_SHORTWAVE=49, ICAR_F_LONGWAVE=50, ICAR_F_CLOUD_FRACTION=51, &
       ICAR_F_ROUGHNESS_Z0=52, ICAR_F_U_10M=53, ICAR_F_V_10M=54, ICAR_F_USTAR=55, ICAR_F_SST=56, ICAR_F_SKIN_TEMPERATURE=57, &
       ICAR_F_SENSIBLE_HEAT=58, ICAR_F_LATENT_HEAT=59, ICAR_F_QSFC=60, ICAR_F_QFX=61, ICAR_F_DZ_INTERFACE=62

  integer(c_int), parameter :: ICAR_N_ADVECTABLE = 11, ICAR_NEIGHBOR_NONE = -1, ICAR_NEIGHBOR_SELF = -2
  integer(c_int), parameter :: ICAR_PBL_SIMPLE = 2      ! kPBL_SIMPLE, icar_constants.f90:355
  integer(c_int), parameter :: ICAR_LSM_BASIC = 1, ICAR_WATER_SIMPLE = 2     ! kLSM_BASIC, kWATER_SIMPLE, icar_constants.f90:358-365
  integer(c_int), parameter :: ICAR_RA_SIMPLE = 2       ! kRA_SIMPLE, icar_constants.f90
  integer(c_int), parameter :: ICAR_CU_BMJ = 5          ! kCU_BMJ, icar_constants.f90:345
  integer(c_int), parameter :: ICAR_PBL_YSU = 3         ! kPBL_YSU, icar_constants.f90:356
  ! enum icar_hip_ysu_array (include/icar_hip.h): the YSU scheme's own arrays, REAL(4) (nx,ny) but for exch_h and the six tendencies
  ! (nx,nz,ny); ICAR_YSU_KPBL is INTEGER(4)
  integer(c_int), parameter :: ICAR_YSU_GROUND_SURF_TEMPERATURE=0, ICAR_YSU_HPBL=1, ICAR_YSU_KPBL=2, ICAR_YSU_EXCH_H=3, ICAR_YSU_PSIM=4, &
       ICAR_YSU_PSIH=5, ICAR_YSU_REGIME=6, ICAR_YSU_RI=7, ICAR_YSU_WINDSPD=8, ICAR_YSU_HOL=9, ICAR_YSU_ZOL=10, ICAR_YSU_GZ1OZ0=11, &
       ICAR_YSU_Z_ATM=12, ICAR_YSU_TEND_TH=13, ICAR_YSU_TEND_QV=14, ICAR_YSU_TEND_QC=15, ICAR_YSU_TEND_QI=16, ICAR_YSU_TEND_U=17, &
       ICAR_YSU_TEND_V=18, ICAR_YSU_N=19
  integer(c_int), parameter :: ICAR_LSM_NOAH = 3        ! kLSM_NOAH, icar_constants.f90
  ! enum icar_hip_noah_array (include/icar_hip.h): the Noah model's arrays, REAL(4) (nx,ny) but VEG_TYPE / SOIL_TYPE, which are INTEGER(4),
  ! and the four soil arrays (nx,4,ny)
  integer(c_int), parameter :: &
       ICAR_NOAH_VEG_TYPE=0, ICAR_NOAH_SOIL_TYPE=1, ICAR_NOAH_VEGFRAC=2, ICAR_NOAH_SOIL_DEEP_TEMPERATURE=3, ICAR_NOAH_SHDMIN=4, ICAR_NOAH_SHDMAX=5, &
       ICAR_NOAH_SNOALB=6, ICAR_NOAH_QGH=7, ICAR_NOAH_CHS=8, ICAR_NOAH_CQS2=9, ICAR_NOAH_RI=10, ICAR_NOAH_CURRENT_PRECIPITATION=11, &
       ICAR_NOAH_GROUND_HEAT_FLUX=12, ICAR_NOAH_SMSTAV=13, ICAR_NOAH_SOIL_TOTALMOISTURE=14, ICAR_NOAH_SFCRUNOFF=15, ICAR_NOAH_UDRUNOFF=16, &
       ICAR_NOAH_ALBEDO=17, ICAR_NOAH_ALBBCK=18, ICAR_NOAH_Z0=19, ICAR_NOAH_EMISS=20, ICAR_NOAH_SNOWC=21, ICAR_NOAH_SNOW_WATER_EQUIVALENT=22, &
       ICAR_NOAH_SNOW_HEIGHT=23, ICAR_NOAH_CANOPY_WATER=24, ICAR_NOAH_CHS2=25, ICAR_NOAH_CHKLOWQ=26, ICAR_NOAH_LAI=27, ICAR_NOAH_SNOTIME=28, &
       ICAR_NOAH_ACSNOM=29, ICAR_NOAH_ACSNOW=30, ICAR_NOAH_SNOPCX=31, ICAR_NOAH_POTEVP=32, ICAR_NOAH_NOAHRES=33, ICAR_NOAH_FLX4=34, ICAR_NOAH_FVB=35, &
       ICAR_NOAH_FBUR=36, ICAR_NOAH_FGSN=37, ICAR_NOAH_SOIL_WATER_CONTENT=38, ICAR_NOAH_SOIL_TEMPERATURE=39, ICAR_NOAH_SH2O=40, ICAR_NOAH_SMCREL=41, &
       ICAR_NOAH_N=42
  ! enum icar_hip_lsm_array (include/icar_hip.h): what the Noah branch of lsm() keeps beside the ICAR_NOAH_* arrays, REAL(4) (nx,ny) but
  ! RAINBL, which is REAL(8)
  integer(c_int), parameter :: &
       ICAR_LSM_TEMPERATURE_2M=0, ICAR_LSM_HUMIDITY_2M=1, ICAR_LSM_LONGWAVE_UP=2, ICAR_LSM_RAINBL=3, ICAR_LSM_Z_ATM=4, ICAR_LSM_LNZ_ATM_TERM=5, &
       ICAR_LSM_BASE_EXCHANGE_TERM=6, ICAR_LSM_N=7
  real(c_float), parameter :: ICAR_CU_NO_STOCHASTIC = -9999.0   ! kNO_STOCHASTIC, icar_constants.f90:340
  ! enum icar_hip_cu_array (include/icar_hip.h): the convection slot's own arrays, REAL(4) (nx,ny) but for the two tendencies (nx,nz,ny)
  integer(c_int), parameter :: ICAR_CU_CLDEFI=0, ICAR_CU_ACC_CONV_PCP=1, ICAR_CU_RAINCV=2, ICAR_CU_CUTOP=3, ICAR_CU_CUBOT=4, &
       ICAR_CU_TEND_TH=5, ICAR_CU_TEND_QV=6, ICAR_CU_N=7
  integer(c_int), parameter :: ICAR_CU_TIEDTKE = 1      ! kCU_TIEDTKE, icar_constants.f90
  ! enum icar_hip_tiedtke_array: the Tiedtke scheme's own arrays: tend%qc, tend%qi (nx,nz,ny), PRATEC (nx,ny) REAL(4), KTYPE (nx,ny) INTEGER(4)
  integer(c_int), parameter :: ICAR_TIEDTKE_TEND_QC=0, ICAR_TIEDTKE_TEND_QI=1, ICAR_TIEDTKE_PRATEC=2, ICAR_TIEDTKE_KTYPE=3, ICAR_TIEDTKE_N=4
  integer(c_int), parameter :: ICAR_CU_NSAS = 4         ! kCU_NSAS, icar_constants.f90
  ! enum icar_hip_forced2d (include/icar_hip.h): the 2-D variables the reference forces, and what hip_forcing2d_get / _set address
  integer(c_int), parameter :: ICAR_FORCED2D_SST = 0, ICAR_FORCED2D_SHORTWAVE = 1, ICAR_FORCED2D_LONGWAVE = 2, &
                               ICAR_FORCED2D_EXTERNAL_PRECIPITATION = 3, ICAR_FORCED2D_N = 4
  integer(c_int), parameter :: ICAR_FORCED2D_DATA = 0, ICAR_FORCED2D_DQDT = 1
  ! enum icar_hip_nsas_array: the NSAS scheme's own REAL(4) arrays: tend%qc, tend%qi (nx,nz,ny), PRATEC, HBOT, HTOP, hpbl (nx,ny)
  integer(c_int), parameter :: ICAR_NSAS_TEND_QC=0, ICAR_NSAS_TEND_QI=1, ICAR_NSAS_PRATEC=2, ICAR_NSAS_HBOT=3, ICAR_NSAS_HTOP=4, ICAR_NSAS_HPBL=5, &
                               ICAR_NSAS_N=6

  ! struct icar_hip_noah_tables_t (include/icar_hip.h) and what a host fills in: pointers to module_sf_noahlsm's own table variables after
  ! SOIL_VEG_GEN_PARM has read them (nrotbl => NROTBL, snuptbl => SNUPTBL, ..., bb => BB, ..., slope_data => SLOPE_DATA) and its scalars
  type, bind(C) :: noah_tables_c
     type(c_ptr) :: nrotbl, snuptbl, rstbl, rgltbl, hstbl, maxalb, emissmintbl, emissmaxtbl, laimintbl, laimaxtbl, z0mintbl, z0maxtbl, &
                    albedomintbl, albedomaxtbl, bb, drysmc, f11, maxsmc, refsmc, satpsi, satdk, satdw, wltsmc, qtz, slope_data
     real(c_float) :: topt_data, cmcmax_data, cfactr_data, rsmax_data, sbeta_data, fxexp_data, csoil_data, salp_data, refdk_data, refkdt_data, &
                      frzk_data, zbot_data, lvcoef_data
     integer(c_int) :: bare, lucats, slcats, slpcats
  end type
  type hip_noah_tables_t
     integer(c_int), pointer, contiguous :: nrotbl(:) => null()
     real(c_float), pointer, contiguous :: snuptbl(:) => null(), rstbl(:) => null(), rgltbl(:) => null(), hstbl(:) => null(), maxalb(:) => null(), &
          emissmintbl(:) => null(), emissmaxtbl(:) => null(), laimintbl(:) => null(), laimaxtbl(:) => null(), z0mintbl(:) => null(), &
          z0maxtbl(:) => null(), albedomintbl(:) => null(), albedomaxtbl(:) => null(), bb(:) => null(), drysmc(:) => null(), f11(:) => null(), &
          maxsmc(:) => null(), refsmc(:) => null(), satpsi(:) => null(), satdk(:) => null(), satdw(:) => null(), wltsmc(:) => null(), &
          qtz(:) => null(), slope_data(:) => null()
     real(c_float) :: topt_data, cmcmax_data, cfactr_data, rsmax_data, sbeta_data, fxexp_data, csoil_data, salp_data, refdk_data, refkdt_data, &
                      frzk_data, zbot_data, lvcoef_data
     integer(c_int) :: bare, lucats, slcats, slpcats
  end type
  !> struct icar_hip_noah_options_t == options%lsm_options as lsm_init reads them for Noah (lsm_driver.f90:633-651, :1280)
  type, bind(C) :: hip_noah_options_t
     integer(c_int) :: urban_category = 13, ice_category = 15, water_category = 17, lake_category = 21
     integer(c_int) :: monthly_vegfrac = 0, monthly_albedo = 0, fndsnowh = 0
     real(c_float)  :: max_swe = 1.0e10
  end type

  !> struct icar_hip_step_config == the members of options_t / grid_t the sub-step loop reads (time_step.f90:440-551)
  type, bind(C) :: hip_step_config_t
     integer(c_int) :: advection = 0, microphysics = 0, mpdata_order = 2, flux_corrected_transport = 1, advect_density = 0
     integer(c_int) :: cfl_strictness = 3
     real(c_float)  :: cfl_reduction_factor = 0.9, dx = 1000.0, mp_update_interval = 0.0
     integer(c_int) :: top_mp_level = 0, halo_size = 1
     integer(c_int) :: its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde
     integer(c_int) :: west_boundary = 1, east_boundary = 1, south_boundary = 1, north_boundary = 1
     integer(c_int) :: diagnostics = 1, prefetch_dt = 1
     integer(c_int) :: n_advect = 0, advect_fields(ICAR_N_ADVECTABLE) = 0
     integer(c_int) :: n_exchange = 0, exchange_fields(ICAR_N_ADVECTABLE) = 0
     integer(c_int) :: n_forced = 0, forced_fields(16) = 0, force_boundaries(16) = 0
  end type

  !> struct icar_hip_lt_options == the members of options%lt_options the linear-wind path reads
  type, bind(C) :: hip_lt_options_t
     integer(c_int) :: buffer, stability_window_size, vert_smooth, variable_N, smooth_nsq
     real(c_float)  :: max_stability, min_stability, N_squared, linear_contribution, linear_update_fraction
     real(c_float)  :: dirmax, dirmin, spdmax, spdmin, nsqmax, nsqmin
     integer(c_int) :: n_dir_values, n_nsq_values, n_spd_values
     real(c_float)  :: minimum_layer_size
  end type

  type :: hip_ctx_t
     type(c_ptr) :: p = c_null_ptr
  end type

  interface
     integer(c_int) function icar_hip_ctx_create(ctx, device, ims, ime, kms, kme, jms, jme) bind(C, name="icar_hip_ctx_create")
       import; type(c_ptr), intent(out) :: ctx; integer(c_int), value :: device, ims, ime, kms, kme, jms, jme
     end function
     integer(c_int) function icar_hip_ctx_destroy(ctx) bind(C, name="icar_hip_ctx_destroy")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_synchronize(ctx) bind(C, name="icar_hip_synchronize")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_make_winds_grid_relative(ctx, update) bind(C, name="icar_hip_make_winds_grid_relative")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: update
     end function
     integer(c_int) function icar_hip_aux_fork(ctx) bind(C, name="icar_hip_aux_fork")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_aux_begin(ctx) bind(C, name="icar_hip_aux_begin")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_aux_end(ctx) bind(C, name="icar_hip_aux_end")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_aux_join(ctx) bind(C, name="icar_hip_aux_join")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_max_courant_device(ctx, dx, dz_levels, d_out) bind(C, name="icar_hip_max_courant_device")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx; real(c_float), intent(in) :: dz_levels(*); type(c_ptr), value :: d_out
     end function
     integer(c_int) function icar_hip_field_upload(ctx, field, host) bind(C, name="icar_hip_field_upload")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: field; type(c_ptr), value :: host
     end function
     integer(c_int) function icar_hip_field_download(ctx, field, host) bind(C, name="icar_hip_field_download")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: field; type(c_ptr), value :: host
     end function
     integer(c_int) function icar_hip_setup_winds(ctx, scheme, dt, dx, advect_density) bind(C, name="icar_hip_setup_winds")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: scheme, advect_density; real(c_float), value :: dt, dx
     end function
     integer(c_int) function icar_hip_advect(ctx, scheme, mpdata_order, fct, advect_density, fields, nfields) bind(C, name="icar_hip_advect")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: scheme, mpdata_order, fct, advect_density, nfields
       integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_mp_simple(ctx, dt, its, ite, jts, jte, kts, kte, err_count) bind(C, name="icar_hip_mp_simple")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
       type(c_ptr), value :: err_count
     end function
     integer(c_int) function icar_hip_thompson_init(ctx, params, flags) bind(C, name="icar_hip_thompson_init")
       import; type(c_ptr), value :: ctx; real(c_float), intent(in) :: params(18); integer(c_int), intent(in) :: flags(2)
     end function
     integer(c_int) function icar_hip_thompson(ctx, dt, its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde) bind(C, name="icar_hip_thompson")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt
       integer(c_int), value :: its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde
     end function
     integer(c_int) function icar_hip_max_courant(ctx, dx, dz_levels, res) bind(C, name="icar_hip_max_courant")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx; real(c_float), intent(in) :: dz_levels(*); real(c_float), intent(out) :: res
     end function
     integer(c_int) function icar_hip_balance_uvw(ctx, dx) bind(C, name="icar_hip_balance_uvw")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx
     end function
     integer(c_int) function icar_hip_max_courant_prefetch(ctx, dx, dz_levels) bind(C, name="icar_hip_max_courant_prefetch")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx; real(c_float), intent(in) :: dz_levels(*)
     end function
     integer(c_int) function icar_hip_winds_valid(ctx) bind(C, name="icar_hip_winds_valid")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_pbl_simple(ctx, dt, its, ite, jts, jte, kts, kte) bind(C, name="icar_hip_pbl_simple")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
     end function
     integer(c_int) function icar_hip_pbl_configure(ctx, boundarylayer) bind(C, name="icar_hip_pbl_configure")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: boundarylayer
     end function
     integer(c_int) function icar_hip_pbl(ctx, dt) bind(C, name="icar_hip_pbl")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt
     end function
     integer(c_int) function icar_hip_pbl_init(ctx, boundarylayer) bind(C, name="icar_hip_pbl_init")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: boundarylayer
     end function
     integer(c_int) function icar_hip_ysu_sfc(ctx) bind(C, name="icar_hip_ysu_sfc")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_ysu(ctx, dt, its, ite, jts, jte, kts, kte) bind(C, name="icar_hip_ysu")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
     end function
     integer(c_int) function icar_hip_ysu_upload(ctx, which, host, count) bind(C, name="icar_hip_ysu_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which; integer(c_size_t), value :: count
     end function
     integer(c_int) function icar_hip_ysu_download(ctx, which, host, count) bind(C, name="icar_hip_ysu_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which; integer(c_size_t), value :: count
     end function
     integer(c_int) function icar_hip_ra_simple(ctx, dt, its, ite, jts, jte, kts, kte, runlw) bind(C, name="icar_hip_ra_simple")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte, runlw
     end function
     integer(c_int) function icar_hip_rad_configure(ctx, radiation) bind(C, name="icar_hip_rad_configure")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: radiation
     end function
     integer(c_int) function icar_hip_rad_calendar(ctx, calendar, year_start_seconds, year_days, next_year_days) bind(C, name="icar_hip_rad_calendar")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: calendar; real(c_double), value :: year_start_seconds, year_days, next_year_days
     end function
     integer(c_int) function icar_hip_rad(ctx, dt) bind(C, name="icar_hip_rad")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt
     end function
     integer(c_int) function icar_hip_lsm_configure(ctx, landsurface, watersurface, update_interval, sh_feedback_fraction, lh_feedback_fraction, &
                                                    sfc_layer_thickness) bind(C, name="icar_hip_lsm_configure")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: landsurface, watersurface, update_interval
       real(c_float), value :: sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness
     end function
     integer(c_int) function icar_hip_diag_10m(ctx) bind(C, name="icar_hip_diag_10m")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_water_simple(ctx) bind(C, name="icar_hip_water_simple")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_apply_fluxes(ctx, dt, its, ite, jts, jte, kts, kte) bind(C, name="icar_hip_apply_fluxes")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
     end function
     integer(c_int) function icar_hip_lsm(ctx, dt) bind(C, name="icar_hip_lsm")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt
     end function
     integer(c_int) function icar_hip_lsm_layers(ctx, nz) bind(C, name="icar_hip_lsm_layers")
       import; type(c_ptr), value :: ctx; integer(c_int) :: nz
     end function
     integer(c_int) function icar_hip_noah_tables(ctx, tables) bind(C, name="icar_hip_noah_tables")
       import; type(c_ptr), value :: ctx; type(noah_tables_c) :: tables
     end function
     integer(c_int) function icar_hip_lsm_init(ctx, landsurface, watersurface, update_interval, sh_feedback_fraction, lh_feedback_fraction, &
                                               sfc_layer_thickness, noah) bind(C, name="icar_hip_lsm_init")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: landsurface, watersurface, update_interval
       real(c_float), value :: sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness; type(hip_noah_options_t) :: noah
     end function
     integer(c_int) function icar_hip_lsm_noah(ctx, lsm_dt, its, ite, jts, jte) bind(C, name="icar_hip_lsm_noah")
       import; type(c_ptr), value :: ctx; real(c_float), value :: lsm_dt; integer(c_int), value :: its, ite, jts, jte
     end function
     integer(c_int) function icar_hip_noah_upload(ctx, which, host) bind(C, name="icar_hip_noah_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_noah_download(ctx, which, host) bind(C, name="icar_hip_noah_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_lsm_noah_couple(ctx) bind(C, name="icar_hip_lsm_noah_couple")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_lsm_upload(ctx, which, host) bind(C, name="icar_hip_lsm_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_lsm_download(ctx, which, host) bind(C, name="icar_hip_lsm_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_cu_configure(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, &
                                                   tend_th_fraction, tend_qi_fraction) bind(C, name="icar_hip_cu_configure")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: convection
       real(c_float), value :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction
     end function
     integer(c_int) function icar_hip_cu_bmj(ctx, dt, its, ite, jts, jte) bind(C, name="icar_hip_cu_bmj")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte
     end function
     integer(c_int) function icar_hip_convect(ctx, dt) bind(C, name="icar_hip_convect")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt
     end function
     integer(c_int) function icar_hip_cu_reset(ctx) bind(C, name="icar_hip_cu_reset")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_cu_upload(ctx, which, host) bind(C, name="icar_hip_cu_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_cu_download(ctx, which, host) bind(C, name="icar_hip_cu_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_cu_init(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, &
                                              tend_th_fraction, tend_qi_fraction, znu) bind(C, name="icar_hip_cu_init")
       import; type(c_ptr), value :: ctx, znu; integer(c_int), value :: convection
       real(c_float), value :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction
     end function
     integer(c_int) function icar_hip_cu_tiedtke(ctx, dt, its, ite, jts, jte) bind(C, name="icar_hip_cu_tiedtke")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte
     end function
     integer(c_int) function icar_hip_tiedtke_upload(ctx, which, host) bind(C, name="icar_hip_tiedtke_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_tiedtke_download(ctx, which, host) bind(C, name="icar_hip_tiedtke_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_convection_init(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, &
                                                      tend_th_fraction, tend_qi_fraction, znu, dx) bind(C, name="icar_hip_convection_init")
       import; type(c_ptr), value :: ctx, znu; integer(c_int), value :: convection
       real(c_float), value :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction, dx
     end function
     integer(c_int) function icar_hip_cu_nsas(ctx, dt, its, ite, jts, jte) bind(C, name="icar_hip_cu_nsas")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte
     end function
     integer(c_int) function icar_hip_nsas_upload(ctx, which, host) bind(C, name="icar_hip_nsas_upload")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_nsas_download(ctx, which, host) bind(C, name="icar_hip_nsas_download")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which
     end function
     integer(c_int) function icar_hip_wsm6_init(ctx) bind(C, name="icar_hip_wsm6_init")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_wsm6(ctx, dt, its, ite, jts, jte, kts, kte) bind(C, name="icar_hip_wsm6")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
     end function
     integer(c_int) function icar_hip_wsm6_tiles(ctx, dt, ntiles, tiles, kts, kte) bind(C, name="icar_hip_wsm6_tiles")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: ntiles, kts, kte
       integer(c_int), intent(in) :: tiles(4,*)
     end function
     integer(c_int) function icar_hip_wsm3_init(ctx) bind(C, name="icar_hip_wsm3_init")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_wsm3(ctx, dt, its, ite, jts, jte, kts, kte) bind(C, name="icar_hip_wsm3")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: its, ite, jts, jte, kts, kte
     end function
     integer(c_int) function icar_hip_diagnostic_update_parts(ctx, parts) bind(C, name="icar_hip_diagnostic_update_parts")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: parts
     end function
     integer(c_int) function icar_hip_diagnostic_update(ctx) bind(C, name="icar_hip_diagnostic_update")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_dqdt_upload(ctx, field, host) bind(C, name="icar_hip_dqdt_upload")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: field; type(c_ptr), value :: host
     end function
     integer(c_int) function icar_hip_apply_forcing(ctx, dt, fields, fb, n, w, e, s, nn) bind(C, name="icar_hip_apply_forcing")
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt; integer(c_int), intent(in) :: fields(*), fb(*)
       integer(c_int), value :: n, w, e, s, nn
     end function
     integer(c_int) function icar_hip_enforce_limits(ctx, fields, n) bind(C, name="icar_hip_enforce_limits")
       import; type(c_ptr), value :: ctx; integer(c_int), intent(in) :: fields(*); integer(c_int), value :: n
     end function
     integer(c_size_t) function icar_hip_halo_count(ctx, dir, halo) bind(C, name="icar_hip_halo_count")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: dir, halo
     end function
     integer(c_int) function icar_hip_halo_pack(ctx, dir, halo, fields, n, dbuf) bind(C, name="icar_hip_halo_pack")
       import; type(c_ptr), value :: ctx, dbuf; integer(c_int), value :: dir, halo, n; integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_halo_unpack(ctx, dir, halo, fields, n, dbuf) bind(C, name="icar_hip_halo_unpack")
       import; type(c_ptr), value :: ctx, dbuf; integer(c_int), value :: dir, halo, n; integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_mp_simple_tiles(ctx, dt, ntiles, tiles, kts, kte, err_count) bind(C, name="icar_hip_mp_simple_tiles")
       import; type(c_ptr), value :: ctx, err_count; real(c_float), value :: dt; integer(c_int), value :: ntiles, kts, kte
       integer(c_int), intent(in) :: tiles(4,*)
     end function
     integer(c_int) function icar_hip_halo_pack_dirs(ctx, ndirs, dirs, halo, fields, n, dbufs) bind(C, name="icar_hip_halo_pack_dirs")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: ndirs, halo, n
       integer(c_int), intent(in) :: dirs(*), fields(*); type(c_ptr), intent(in) :: dbufs(*)
     end function
     integer(c_int) function icar_hip_halo_unpack_dirs(ctx, ndirs, dirs, halo, fields, n, dbufs) bind(C, name="icar_hip_halo_unpack_dirs")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: ndirs, halo, n
       integer(c_int), intent(in) :: dirs(*), fields(*); type(c_ptr), intent(in) :: dbufs(*)
     end function
     integer(c_int) function icar_hip_thompson_tiles(ctx, dt, ntiles, tiles, kts, kte, ids, ide, jds, jde, kds, kde) &
          bind(C, name="icar_hip_thompson_tiles")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dt; integer(c_int), value :: ntiles, kts, kte, ids, ide, jds, jde, kds, kde
       integer(c_int), intent(in) :: tiles(4,*)
     end function
     integer(c_int) function icar_hip_mass_conservative_acceleration(ctx, update) bind(C, name="icar_hip_mass_conservative_acceleration")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: update
     end function
     integer(c_int) function icar_hip_iterative_winds_correct_w(ctx, update) bind(C, name="icar_hip_iterative_winds_correct_w")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: update
     end function
     integer(c_int) function icar_hip_iterative_winds_sweep(ctx, dx, nsweeps, update) bind(C, name="icar_hip_iterative_winds_sweep")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx; integer(c_int), value :: nsweeps, update
     end function
     integer(c_int) function icar_hip_balance_uvw_update(ctx, dx) bind(C, name="icar_hip_balance_uvw_update")
       import; type(c_ptr), value :: ctx; real(c_float), value :: dx
     end function
     integer(c_int) function icar_hip_linwinds_setup(ctx, opt, terrain, nxg, nyg, ids, jds, dx) bind(C, name="icar_hip_linwinds_setup")
       import; type(c_ptr), value :: ctx; type(hip_lt_options_t), intent(in) :: opt; real(c_float), intent(in) :: terrain(*)
       integer(c_int), value :: nxg, nyg, ids, jds; real(c_float), value :: dx
     end function
     integer(c_int) function icar_hip_linwinds_build_lut(ctx, z_bottom, z_top, nz) bind(C, name="icar_hip_linwinds_build_lut")
       import; type(c_ptr), value :: ctx; real(c_float), intent(in) :: z_bottom(*), z_top(*); integer(c_int), value :: nz
     end function
     integer(c_int) function icar_hip_spatial_winds(ctx, update) bind(C, name="icar_hip_spatial_winds")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: update
     end function
     type(c_ptr) function icar_hip_last_error() bind(C, name="icar_hip_last_error")
       import
     end function
     ! ---- H1 transport + co_min, and the sub-step loop itself (comm.hip, timestep.hip) ----
     integer(c_int) function icar_hip_comm_unique_id(uid) bind(C, name="icar_hip_comm_unique_id")
       import; character(kind=c_char) :: uid(128)
     end function
     integer(c_int) function icar_hip_comm_init(ctx, nranks, rank, uid, neighbors) bind(C, name="icar_hip_comm_init")
       import; type(c_ptr), value :: ctx, uid; integer(c_int), value :: nranks, rank; integer(c_int), intent(in) :: neighbors(4)
     end function
     integer(c_int) function icar_hip_comm_init_host(ctx, nranks, rank, shm_name, slot_bytes, neighbors) bind(C, name="icar_hip_comm_init_host")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: nranks, rank; character(kind=c_char), intent(in) :: shm_name(*)
       integer(c_size_t), value :: slot_bytes; integer(c_int), intent(in) :: neighbors(4)
     end function
     integer(c_int) function icar_hip_comm_destroy(ctx) bind(C, name="icar_hip_comm_destroy")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_halo_send(ctx, halo, fields, n) bind(C, name="icar_hip_halo_send")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: halo, n; integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_halo_retrieve(ctx, halo, fields, n) bind(C, name="icar_hip_halo_retrieve")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: halo, n; integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_co_min(ctx, v) bind(C, name="icar_hip_co_min")
       import; type(c_ptr), value :: ctx; real(c_double), intent(inout) :: v
     end function
     integer(c_int) function icar_hip_forcing_configure(ctx, mass, u, v, nsmooth, forcing_z, domain_z, time_varying_z) bind(C, name="icar_hip_forcing_configure")
       import; type(c_ptr), value :: ctx, mass, u, v, forcing_z, domain_z; integer(c_int), value :: nsmooth, time_varying_z
     end function
     integer(c_int) function icar_hip_forcing_upload(ctx, field, lo, nx_f, nz_f, ny_f) bind(C, name="icar_hip_forcing_upload")
       import; type(c_ptr), value :: ctx, lo; integer(c_int), value :: field, nx_f, nz_f, ny_f
     end function
     integer(c_int) function icar_hip_forcing_download(ctx, field, lo, count) bind(C, name="icar_hip_forcing_download")
       import; type(c_ptr), value :: ctx, lo; integer(c_int), value :: field; integer(c_size_t), value :: count
     end function
     integer(c_int) function icar_hip_interpolate_forcing(ctx, fields, n, pressure_field, theta_field, update) bind(C, name="icar_hip_interpolate_forcing")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n, pressure_field, theta_field, update; integer(c_int), intent(in) :: fields(*)
     end function
     integer(c_int) function icar_hip_update_delta_fields(ctx, fields, n, dt_seconds) bind(C, name="icar_hip_update_delta_fields")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n; integer(c_int), intent(in) :: fields(*); real(c_double), value :: dt_seconds
     end function
     integer(c_int) function icar_hip_forcing_step(ctx, fields, n, pressure_field, theta_field, windtype, wind_iterations, dx, halo, dt_seconds) &
                                                   bind(C, name="icar_hip_forcing_step")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n, pressure_field, theta_field, windtype, wind_iterations, halo
       integer(c_int), intent(in) :: fields(*); real(c_float), value :: dx; real(c_double), value :: dt_seconds
     end function
     integer(c_int) function icar_hip_forcing2d_upload(ctx, which, lo, nx_f, ny_f) bind(C, name="icar_hip_forcing2d_upload")
       import; type(c_ptr), value :: ctx, lo; integer(c_int), value :: which, nx_f, ny_f
     end function
     integer(c_int) function icar_hip_forcing2d_download(ctx, which, lo, count) bind(C, name="icar_hip_forcing2d_download")
       import; type(c_ptr), value :: ctx, lo; integer(c_int), value :: which; integer(c_size_t), value :: count
     end function
     integer(c_int) function icar_hip_interpolate_forcing_2d(ctx, which, n, update) bind(C, name="icar_hip_interpolate_forcing_2d")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n, update; integer(c_int), intent(in) :: which(*)
     end function
     integer(c_int) function icar_hip_update_delta_fields_2d(ctx, which, n, dt_seconds) bind(C, name="icar_hip_update_delta_fields_2d")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n; integer(c_int), intent(in) :: which(*); real(c_double), value :: dt_seconds
     end function
     integer(c_int) function icar_hip_apply_forcing_2d(ctx, dt_seconds) bind(C, name="icar_hip_apply_forcing_2d")
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt_seconds
     end function
     integer(c_int) function icar_hip_forcing2d_enable(ctx, which, n) bind(C, name="icar_hip_forcing2d_enable")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: n; integer(c_int), intent(in) :: which(*)
     end function
     integer(c_int) function icar_hip_forcing2d_get(ctx, which, what, host) bind(C, name="icar_hip_forcing2d_get")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which, what
     end function
     integer(c_int) function icar_hip_forcing2d_set(ctx, which, what, host) bind(C, name="icar_hip_forcing2d_set")
       import; type(c_ptr), value :: ctx, host; integer(c_int), value :: which, what
     end function
     integer(c_int) function icar_hip_update_winds(ctx, windtype, wind_iterations, dx, halo, update) bind(C, name="icar_hip_update_winds")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: windtype, wind_iterations, halo, update; real(c_float), value :: dx
     end function
     integer(c_int) function icar_hip_exchange_uv(ctx, halo, update) bind(C, name="icar_hip_exchange_uv")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: halo, update
     end function
     integer(c_int) function icar_hip_comm_ranks(ctx, nranks) bind(C, name="icar_hip_comm_ranks")
       import; type(c_ptr), value :: ctx; integer(c_int), intent(out) :: nranks
     end function
     integer(c_int) function icar_hip_mpdata_exact(ctx, on) bind(C, name="icar_hip_mpdata_exact")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: on
     end function
     integer(c_int) function icar_hip_halo_selfcheck(ctx, halo, n_bad) bind(C, name="icar_hip_halo_selfcheck")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: halo; integer(c_int), intent(out) :: n_bad
     end function
     integer(c_int) function icar_hip_step_configure(ctx, cfg, dz_levels) bind(C, name="icar_hip_step_configure")
       import; type(c_ptr), value :: ctx; type(hip_step_config_t), intent(in) :: cfg; real(c_float), intent(in) :: dz_levels(*)
     end function
     integer(c_int) function icar_hip_model_time_set(ctx, seconds) bind(C, name="icar_hip_model_time_set")
       import; type(c_ptr), value :: ctx; real(c_double), value :: seconds
     end function
     real(c_double) function icar_hip_model_time(ctx) bind(C, name="icar_hip_model_time")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_mp_reset(ctx) bind(C, name="icar_hip_mp_reset")
       import; type(c_ptr), value :: ctx
     end function
     integer(c_int) function icar_hip_compute_dt(ctx, dt) bind(C, name="icar_hip_compute_dt")
       import; type(c_ptr), value :: ctx; real(c_double), intent(out) :: dt
     end function
     integer(c_int) function icar_hip_update_dt(ctx, dt) bind(C, name="icar_hip_update_dt")
       import; type(c_ptr), value :: ctx; real(c_double), intent(out) :: dt
     end function
     integer(c_int) function icar_hip_mp(ctx, dt, halo, subset) bind(C, name="icar_hip_mp")
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt; integer(c_int), value :: halo, subset
     end function
     integer(c_int) function icar_hip_advect_step(ctx, dt) bind(C, name="icar_hip_advect_step")
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt
     end function
     integer(c_int) function icar_hip_substep(ctx, dt, enforce) bind(C, name="icar_hip_substep")
       import; type(c_ptr), value :: ctx; real(c_double), value :: dt; integer(c_int), value :: enforce
     end function
     integer(c_int) function icar_hip_step(ctx, end_time, nsteps) bind(C, name="icar_hip_step")
       import; type(c_ptr), value :: ctx; real(c_double), value :: end_time; integer(c_int), intent(out) :: nsteps
     end function
     integer(c_int) function icar_hip_step_n(ctx, nsteps, dt_last) bind(C, name="icar_hip_step_n")
       import; type(c_ptr), value :: ctx; integer(c_int), value :: nsteps; real(c_double), intent(out) :: dt_last
     end function
  end interface

contains

  !> hand the library the options_t / grid_t members the loop reads; then hip_step == step(domain, end_time, options)
  subroutine hip_step_configure(ctx, cfg, dz_levels)
    type(hip_ctx_t), intent(in) :: ctx
    type(hip_step_config_t), intent(in) :: cfg
    real(c_float), intent(in) :: dz_levels(:)
    call check(icar_hip_step_configure(ctx%p, cfg, dz_levels), "step_configure")
  end subroutine

  !> update_dt (time_step.f90:375-423): compute_dt + co_min over the images + the 120 s cap
  function hip_update_dt(ctx) result(dt)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double) :: dt
    call check(icar_hip_update_dt(ctx%p, dt), "update_dt")
  end function

  function hip_compute_dt(ctx) result(dt)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double) :: dt
    call check(icar_hip_compute_dt(ctx%p, dt), "compute_dt")
  end function

  !> one pass of time_step.f90:474-539 (diagnostic_update ... enforce_limits), two streams inside the library
  subroutine hip_substep(ctx, dt, enforce_limits)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(in) :: dt
    logical, intent(in) :: enforce_limits
    call check(icar_hip_substep(ctx%p, dt, merge(1_c_int,0_c_int,enforce_limits)), "substep")
  end subroutine

  !> step(domain, end_time, options) (time_step.f90:440-551); the model clock lives in the context (hip_model_time)
  function hip_step(ctx, end_time) result(nsteps)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(in) :: end_time
    integer :: nsteps
    integer(c_int) :: n
    call check(icar_hip_step(ctx%p, end_time, n), "step"); nsteps = n
  end function

  !> nsteps sub-steps (update_dt -> substep -> clock += dt) without an end time; returns the last dt
  function hip_step_n(ctx, nsteps) result(dt)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: nsteps
    real(c_double) :: dt
    call check(icar_hip_step_n(ctx%p, int(nsteps,c_int), dt), "step_n")
  end function

  !> mp(domain, options, dt, halo, subset) (mp_driver.f90:673-772); absent halo / subset like the reference's optionals
  subroutine hip_mp(ctx, dt, halo, subset)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(in) :: dt
    integer, intent(in), optional :: halo, subset
    integer(c_int) :: h, s
    h = -1; s = -1
    if (present(halo)) h = halo
    if (present(subset)) s = subset
    call check(icar_hip_mp(ctx%p, dt, h, s), "mp")
  end subroutine

  !> advect(domain, options, dt) (advection_driver.f90:51-77)
  subroutine hip_advect_step(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(in) :: dt
    call check(icar_hip_advect_step(ctx%p, dt), "advect_step")
  end subroutine

  !> options%physics%boundarylayer for the sub-step loop: 0, 1 (kPBL_BASIC: nothing runs) or ICAR_PBL_SIMPLE; 3 (YSU) stops: hip_pbl_init selects it
  subroutine hip_pbl_configure(ctx, boundarylayer)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: boundarylayer
    call check(icar_hip_pbl_configure(ctx%p, int(boundarylayer,c_int)), "pbl_configure")
  end subroutine

  !> pbl_init(domain, options) (pbl_driver.f90:106-195): 0, 1, 2 as hip_pbl_configure; ICAR_PBL_YSU makes z_atm, gz1oz0, zol, hol from
  !! ICAR_F_Z, ICAR_F_TERRAIN, ICAR_F_ROUGHNESS_Z0 (ICAR_F_LAND_MASK must be there too), zeroes the tendencies, allocates the workspace
  subroutine hip_pbl_init(ctx, boundarylayer)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: boundarylayer
    call check(icar_hip_pbl_init(ctx%p, int(boundarylayer,c_int)), "pbl_init")
  end subroutine

  !> pbl_driver.f90:227-254 alone: the 10 m wind speed with its floor, calc_Richardson_nr, da_sfc_wtq over the whole memory
  subroutine hip_ysu_sfc(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_ysu_sfc(ctx%p), "ysu_sfc")
  end subroutine

  !> `call ysu(...)` alone (pbl_driver.f90:257-323); kte is the model's (lowered by one inside); the tendencies stay in place
  subroutine hip_ysu(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_ysu(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                            int(kts,c_int), int(kte,c_int)), "ysu")
  end subroutine

  !> the scheme's own arrays by ICAR_YSU_*: a contiguous REAL(4) array of (nx,ny), or (nx,nz,ny) for exch_h and the tendencies
  subroutine hip_ysu_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(..)
    call check(icar_hip_ysu_upload(ctx%p, which, c_loc(a), int(size(a),c_size_t)), "ysu_upload")
  end subroutine

  subroutine hip_ysu_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(..)
    call check(icar_hip_ysu_download(ctx%p, which, c_loc(a), int(size(a),c_size_t)), "ysu_download")
  end subroutine

  !> domain%kpbl (INTEGER) from ICAR_YSU_KPBL
  subroutine hip_ysu_download_kpbl(ctx, kpbl)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(inout), target, contiguous :: kpbl(:,:)
    call check(icar_hip_ysu_download(ctx%p, ICAR_YSU_KPBL, c_loc(kpbl), int(size(kpbl),c_size_t)), "ysu_download")
  end subroutine

  !> pbl(domain, options, dt) (pbl_driver.f90:197-354) on the tile of hip_step_configure; dt = real(dt%seconds())
  subroutine hip_pbl(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    call check(icar_hip_pbl(ctx%p, real(dt,c_float)), "pbl")
  end subroutine

  !> simple_pbl (pbl_simple.f90:69-141) on the context's fields; ICAR_F_TERRAIN and (optionally) ICAR_F_LAND_MASK uploaded once
  subroutine hip_pbl_simple(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_pbl_simple(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                                   int(kts,c_int), int(kte,c_int)), "pbl_simple")
  end subroutine

  !> options%physics%radiation for the sub-step loop: 0, 1 (kRA_BASIC: nothing runs) or ICAR_RA_SIMPLE; 3 (RRTMG) stops
  subroutine hip_rad_configure(ctx, radiation)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: radiation
    call check(icar_hip_rad_configure(ctx%p, int(radiation,c_int)), "rad_configure")
  end subroutine

  !> what Time_type%day_of_year / %year_fraction (time_obj.f90:404-480) need of domain%model_time: calendar (0 gregorian,
  !! 1 noleap, 2 360-day), the library clock's value at 1 January 00:00 of the model time's year, that year's and the next one's days
  subroutine hip_rad_calendar(ctx, calendar, year_start_seconds, year_days, next_year_days)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: calendar
    double precision, intent(in) :: year_start_seconds, year_days, next_year_days
    call check(icar_hip_rad_calendar(ctx%p, int(calendar,c_int), real(year_start_seconds,c_double), real(year_days,c_double), &
                                     real(next_year_days,c_double)), "rad_calendar")
  end subroutine

  !> rad(domain, options, dt) (ra_driver.f90:197-285) on the tile of hip_step_configure; dt = real(dt%seconds())
  subroutine hip_rad(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    call check(icar_hip_rad(ctx%p, real(dt,c_float)), "rad")
  end subroutine

  !> ra_simple (ra_simple.f90:191-272) on the context's fields; ICAR_F_LATITUDE / ICAR_F_LONGITUDE uploaded once (hip_upload_2d)
  subroutine hip_ra_simple(ctx, dt, its, ite, jts, jte, kts, kte, runlw)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    logical, intent(in) :: runlw
    call check(icar_hip_ra_simple(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                                  int(kts,c_int), int(kte,c_int), merge(1_c_int, 0_c_int, runlw)), "ra_simple")
  end subroutine

  !> lsm_init (lsm_driver.f90:522-611, :991-1000): options%physics%landsurface (0 or ICAR_LSM_BASIC; 2 stops as the reference does,
  !! 3 and 4 are not built), %watersurface (0, 1 or ICAR_WATER_SIMPLE; 3 is not built) and options%lsm_options; resets the update gate
  subroutine hip_lsm_configure(ctx, landsurface, watersurface, update_interval, sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: landsurface, watersurface, update_interval
    real, intent(in) :: sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness
    call check(icar_hip_lsm_configure(ctx%p, int(landsurface,c_int), int(watersurface,c_int), int(update_interval,c_int), &
                                      real(sh_feedback_fraction,c_float), real(lh_feedback_fraction,c_float), real(sfc_layer_thickness,c_float)), "lsm_configure")
  end subroutine

  !> u_10m, v_10m and ustar of diagnostic_update (time_step.f90:143-161); ICAR_F_ROUGHNESS_Z0 uploaded
  subroutine hip_diag_10m(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_diag_10m(ctx%p), "diag_10m")
  end subroutine

  !> the gated block of lsm with watersurface = kWATER_SIMPLE (lsm_driver.f90:1028-1073, water_simple.f90:83-136)
  subroutine hip_water_simple(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_water_simple(ctx%p), "water_simple")
  end subroutine

  !> apply_fluxes(domain, dt) (lsm_driver.f90:361-423) on an explicit tile
  subroutine hip_apply_fluxes(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_apply_fluxes(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                                     int(kts,c_int), int(kte,c_int)), "apply_fluxes")
  end subroutine

  !> lsm(domain, options, dt) (lsm_driver.f90:1005-1554) on the tile of hip_step_configure; dt = real(dt%seconds())
  subroutine hip_lsm(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    call check(icar_hip_lsm(ctx%p, real(dt,c_float)), "lsm")
  end subroutine

  !> apply_fluxes' nz (the levels below sfc_layer_thickness) for the configured tile
  function hip_lsm_layers(ctx) result(nz)
    type(hip_ctx_t), intent(in) :: ctx
    integer :: nz
    integer(c_int) :: n
    call check(icar_hip_lsm_layers(ctx%p, n), "lsm_layers")
    nz = int(n)
  end function

  !> SOIL_VEG_GEN_PARM's results (lsm_noahdrv.f90:1199-1432) to the device: t's pointers are associated with module_sf_noahlsm's arrays
  subroutine hip_noah_tables(ctx, t)
    type(hip_ctx_t), intent(in) :: ctx
    type(hip_noah_tables_t), intent(in) :: t
    type(noah_tables_c) :: c
    c%nrotbl = c_loc(t%nrotbl); c%snuptbl = c_loc(t%snuptbl); c%rstbl = c_loc(t%rstbl); c%rgltbl = c_loc(t%rgltbl); c%hstbl = c_loc(t%hstbl)
    c%maxalb = c_loc(t%maxalb); c%emissmintbl = c_loc(t%emissmintbl); c%emissmaxtbl = c_loc(t%emissmaxtbl); c%laimintbl = c_loc(t%laimintbl)
    c%laimaxtbl = c_loc(t%laimaxtbl); c%z0mintbl = c_loc(t%z0mintbl); c%z0maxtbl = c_loc(t%z0maxtbl); c%albedomintbl = c_loc(t%albedomintbl)
    c%albedomaxtbl = c_loc(t%albedomaxtbl); c%bb = c_loc(t%bb); c%drysmc = c_loc(t%drysmc); c%f11 = c_loc(t%f11); c%maxsmc = c_loc(t%maxsmc)
    c%refsmc = c_loc(t%refsmc); c%satpsi = c_loc(t%satpsi); c%satdk = c_loc(t%satdk); c%satdw = c_loc(t%satdw); c%wltsmc = c_loc(t%wltsmc)
    c%qtz = c_loc(t%qtz); c%slope_data = c_loc(t%slope_data)
    c%topt_data = t%topt_data; c%cmcmax_data = t%cmcmax_data; c%cfactr_data = t%cfactr_data; c%rsmax_data = t%rsmax_data; c%sbeta_data = t%sbeta_data
    c%fxexp_data = t%fxexp_data; c%csoil_data = t%csoil_data; c%salp_data = t%salp_data; c%refdk_data = t%refdk_data; c%refkdt_data = t%refkdt_data
    c%frzk_data = t%frzk_data; c%zbot_data = t%zbot_data; c%lvcoef_data = t%lvcoef_data
    c%bare = t%bare; c%lucats = t%lucats; c%slcats = t%slcats; c%slpcats = t%slpcats
    call check(icar_hip_noah_tables(ctx%p, c), "noah_tables")
  end subroutine

  !> lsm_init (lsm_driver.f90:522-711) with every landsurface that is built: 0 and ICAR_LSM_BASIC as hip_lsm_configure; ICAR_LSM_NOAH after
  !! hip_noah_tables and the uploads of the domain's arrays (hip_noah_upload)
  subroutine hip_lsm_init(ctx, landsurface, watersurface, update_interval, sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness, noah)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: landsurface, watersurface, update_interval
    real, intent(in) :: sh_feedback_fraction, lh_feedback_fraction, sfc_layer_thickness
    type(hip_noah_options_t), intent(in) :: noah
    type(hip_noah_options_t) :: n
    n = noah
    call check(icar_hip_lsm_init(ctx%p, int(landsurface,c_int), int(watersurface,c_int), int(update_interval,c_int), real(sh_feedback_fraction,c_float), &
                                 real(lh_feedback_fraction,c_float), real(sfc_layer_thickness,c_float), n), "lsm_init")
  end subroutine

  !> the call of lsm_noah alone (lsm_driver.f90:1210-1278) on a tile
  subroutine hip_lsm_noah(ctx, lsm_dt, its, ite, jts, jte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: lsm_dt
    integer, intent(in) :: its, ite, jts, jte
    call check(icar_hip_lsm_noah(ctx%p, real(lsm_dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int)), "lsm_noah")
  end subroutine

  !> the Noah model's arrays by ICAR_NOAH_*: REAL(4) (nx,ny) or (nx,4,ny); ICAR_NOAH_VEG_TYPE / _SOIL_TYPE through the _int pair
  subroutine hip_noah_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(..)
    call check(icar_hip_noah_upload(ctx%p, which, c_loc(a)), "noah_upload")
  end subroutine

  subroutine hip_noah_upload_int(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    integer(c_int), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_noah_upload(ctx%p, which, c_loc(a)), "noah_upload")
  end subroutine

  subroutine hip_noah_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(..)
    call check(icar_hip_noah_download(ctx%p, which, c_loc(a)), "noah_download")
  end subroutine

  subroutine hip_noah_download_int(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    integer(c_int), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_noah_download(ctx%p, which, c_loc(a)), "noah_download")
  end subroutine

  !> what lsm_init does for Noah beside hip_lsm_init's part (lsm_driver.f90:566, :583-587, :592-596, :602-603, :610-611, :992-997), after
  !! hip_lsm_init(.., ICAR_LSM_NOAH, ..): from here on hip_lsm and the step entry points run the Noah branch of lsm() (:1028-1546)
  subroutine hip_lsm_noah_couple(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_lsm_noah_couple(ctx%p), "lsm_noah_couple")
  end subroutine

  !> the arrays of that branch by ICAR_LSM_*: REAL(4) (nx,ny); ICAR_LSM_RAINBL, REAL(8), through the _r8 pair
  subroutine hip_lsm_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_lsm_upload(ctx%p, which, c_loc(a)), "lsm_upload")
  end subroutine

  subroutine hip_lsm_upload_r8(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_double), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_lsm_upload(ctx%p, which, c_loc(a)), "lsm_upload")
  end subroutine

  subroutine hip_lsm_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_lsm_download(ctx%p, which, c_loc(a)), "lsm_download")
  end subroutine

  subroutine hip_lsm_download_r8(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_double), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_lsm_download(ctx%p, which, c_loc(a)), "lsm_download")
  end subroutine

  !> init_convection (cu_driver.f90:97-253): options%physics%convection (0 or ICAR_CU_BMJ; Tiedtke goes through hip_cu_init, NSAS through hip_convection_init, 2 and 3 have no
  !! branch in the reference) and options%cu_options (stochastic_cu must be kNO_STOCHASTIC; a negative fraction inherits tendency_fraction)
  subroutine hip_cu_configure(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: convection
    real, intent(in) :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction
    call check(icar_hip_cu_configure(ctx%p, int(convection,c_int), real(stochastic_cu,c_float), real(tendency_fraction,c_float), &
                                     real(tend_qv_fraction,c_float), real(tend_qc_fraction,c_float), real(tend_th_fraction,c_float), &
                                     real(tend_qi_fraction,c_float)), "cu_configure")
  end subroutine

  !> the call of BMJDRV alone (cu_driver.f90:434-465) on a range of columns
  subroutine hip_cu_bmj(ctx, dt, its, ite, jts, jte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte
    call check(icar_hip_cu_bmj(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int)), "cu_bmj")
  end subroutine

  !> convect(domain, options, dt) (cu_driver.f90:255-514) on the tile of hip_step_configure; dt = real(dt%seconds())
  subroutine hip_convect(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    call check(icar_hip_convect(ctx%p, real(dt,c_float)), "convect")
  end subroutine

  !> CLDEFI = AVGEFI, accumulated_convective_pcp = 0
  subroutine hip_cu_reset(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_cu_reset(ctx%p), "cu_reset")
  end subroutine

  !> the slot's own arrays by ICAR_CU_*: a contiguous REAL(4) array of (nx,ny), or (nx,nz,ny) for the two tendencies
  subroutine hip_cu_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(..)
    call check(icar_hip_cu_upload(ctx%p, which, c_loc(a)), "cu_upload")
  end subroutine

  subroutine hip_cu_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(..)
    call check(icar_hip_cu_download(ctx%p, which, c_loc(a)), "cu_download")
  end subroutine

  !> init_convection with every scheme that is built: 0 and ICAR_CU_BMJ as hip_cu_configure; ICAR_CU_TIEDTKE takes domain%znu(kms:kme)
  subroutine hip_cu_init(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction, znu)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: convection
    real, intent(in) :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction
    real(c_float), intent(in), target, contiguous :: znu(:)
    call check(icar_hip_cu_init(ctx%p, int(convection,c_int), real(stochastic_cu,c_float), real(tendency_fraction,c_float), &
                                real(tend_qv_fraction,c_float), real(tend_qc_fraction,c_float), real(tend_th_fraction,c_float), &
                                real(tend_qi_fraction,c_float), c_loc(znu)), "cu_init")
  end subroutine

  !> the call of CU_TIEDTKE alone (cu_driver.f90:303-330) on a range of columns
  subroutine hip_cu_tiedtke(ctx, dt, its, ite, jts, jte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte
    call check(icar_hip_cu_tiedtke(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int)), "cu_tiedtke")
  end subroutine

  !> the Tiedtke scheme's REAL(4) arrays by ICAR_TIEDTKE_*: (nx,nz,ny) for the two tendencies, (nx,ny) for PRATEC
  subroutine hip_tiedtke_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(..)
    call check(icar_hip_tiedtke_upload(ctx%p, which, c_loc(a)), "tiedtke_upload")
  end subroutine

  subroutine hip_tiedtke_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(..)
    call check(icar_hip_tiedtke_download(ctx%p, which, c_loc(a)), "tiedtke_download")
  end subroutine

  !> KTYPE (nx,ny) INTEGER(4) of the last call
  subroutine hip_tiedtke_download_ktype(ctx, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_tiedtke_download(ctx%p, ICAR_TIEDTKE_KTYPE, c_loc(a)), "tiedtke_download")
  end subroutine

  !> init_convection with every scheme that is built: 0, ICAR_CU_BMJ and ICAR_CU_TIEDTKE as hip_cu_init; ICAR_CU_NSAS takes domain%dx
  subroutine hip_convection_init(ctx, convection, stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, &
                                 tend_qi_fraction, znu, dx)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: convection
    real, intent(in) :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction, dx
    real(c_float), intent(in), target, contiguous :: znu(:)
    call check(icar_hip_convection_init(ctx%p, int(convection,c_int), real(stochastic_cu,c_float), real(tendency_fraction,c_float), &
                                        real(tend_qv_fraction,c_float), real(tend_qc_fraction,c_float), real(tend_th_fraction,c_float), &
                                        real(tend_qi_fraction,c_float), c_loc(znu), real(dx,c_float)), "convection_init")
  end subroutine

  !> the call of cu_nsas alone (cu_driver.f90:363-417) on a range of columns
  subroutine hip_cu_nsas(ctx, dt, its, ite, jts, jte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte
    call check(icar_hip_cu_nsas(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int)), "cu_nsas")
  end subroutine

  !> the NSAS scheme's REAL(4) arrays by ICAR_NSAS_*: (nx,nz,ny) for the two tendencies, (nx,ny) for PRATEC, HBOT, HTOP and hpbl
  subroutine hip_nsas_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(..)
    call check(icar_hip_nsas_upload(ctx%p, which, c_loc(a)), "nsas_upload")
  end subroutine

  subroutine hip_nsas_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(..)
    call check(icar_hip_nsas_download(ctx%p, which, c_loc(a)), "nsas_download")
  end subroutine

  subroutine hip_mp_reset(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_mp_reset(ctx%p), "mp_reset")
  end subroutine

  function hip_model_time(ctx) result(t)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double) :: t
    t = icar_hip_model_time(ctx%p)
  end function

  subroutine hip_set_model_time(ctx, seconds)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(in) :: seconds
    call check(icar_hip_model_time_set(ctx%p, seconds), "model_time_set")
  end subroutine

  !> image 1 calls this and co_broadcasts the 128 bytes; every image then calls hip_comm_init (RCCL, one GPU per image)
  subroutine hip_comm_unique_id(uid)
    character(kind=c_char), intent(out) :: uid(128)
    call check(icar_hip_comm_unique_id(uid), "comm_unique_id")
  end subroutine

  !> neighbors(1:4) = 0-based rank (= image - 1) of the north, south, east, west neighbour, ICAR_NEIGHBOR_NONE on a domain boundary
  subroutine hip_comm_init(ctx, nranks, rank, uid, neighbors)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: nranks, rank
    character(kind=c_char), intent(in), target :: uid(128)
    integer(c_int), intent(in) :: neighbors(4)
    call check(icar_hip_comm_init(ctx%p, int(nranks,c_int), int(rank,c_int), c_loc(uid), neighbors), "comm_init")
  end subroutine

  !> one image without peers (edges may wrap: ICAR_NEIGHBOR_SELF)
  subroutine hip_comm_init_local(ctx, neighbors)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: neighbors(4)
    call check(icar_hip_comm_init(ctx%p, 1_c_int, 0_c_int, c_null_ptr, neighbors), "comm_init")
  end subroutine

  !> the same entry points staged through POSIX shared memory: several images on one GPU (functional path)
  subroutine hip_comm_init_host(ctx, nranks, rank, shm_name, slot_bytes, neighbors)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: nranks, rank
    character(len=*), intent(in) :: shm_name
    integer(c_size_t), intent(in) :: slot_bytes
    integer(c_int), intent(in) :: neighbors(4)
    call check(icar_hip_comm_init_host(ctx%p, int(nranks,c_int), int(rank,c_int), trim(shm_name)//c_null_char, slot_bytes, neighbors), "comm_init_host")
  end subroutine

  subroutine hip_comm_destroy(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_comm_destroy(ctx%p), "comm_destroy")
  end subroutine

  !> domain%halo_send / halo_retrieve (domain_obj.f90:109-143) for the listed exchangeables, one message per neighbour
  subroutine hip_halo_send(ctx, halo, fields)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: halo
    integer(c_int), intent(in) :: fields(:)
    call check(icar_hip_halo_send(ctx%p, int(halo,c_int), fields, int(size(fields),c_int)), "halo_send")
  end subroutine
  subroutine hip_halo_retrieve(ctx, halo, fields)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: halo
    integer(c_int), intent(in) :: fields(:)
    call check(icar_hip_halo_retrieve(ctx%p, int(halo,c_int), fields, int(size(fields),c_int)), "halo_retrieve")
  end subroutine

  !> call co_min(seconds) (time_step.f90:413)
  subroutine hip_co_min(ctx, v)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_double), intent(inout) :: v
    call check(icar_hip_co_min(ctx%p, v), "co_min")
  end subroutine

  !> num_images() as the transport reports it (ncclCommCount / the shared segment's header)
  integer function hip_comm_ranks(ctx) result(n)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int) :: nr
    call check(icar_hip_comm_ranks(ctx%p, nr), "comm_ranks")
    n = int(nr)
  end function

  !> one exchange of a rank-stamped field, verified on the device (exchangeable_obj.f90:138-356); returns the number of halo
  !! cells that do not carry their neighbour's stamp.  Collective.
  integer function hip_halo_selfcheck(ctx, halo) result(n_bad)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: halo
    integer(c_int) :: nb
    call check(icar_hip_halo_selfcheck(ctx%p, int(halo,c_int), nb), "halo_selfcheck")
    n_bad = int(nb)
  end function

  !> MPDATA's corrective iterations in the operation order of adv_mpdata.f90 (bit-identical to the CPU reference, ~4x the
  !! advection time of the fused kernel); .false. = the fused kernel (default)
  subroutine hip_mpdata_exact(ctx, on)
    type(hip_ctx_t), intent(in) :: ctx
    logical, intent(in) :: on
    call check(icar_hip_mpdata_exact(ctx%p, merge(1_c_int, 0_c_int, on)), "mpdata_exact")
  end subroutine

  subroutine check(rc, what)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: what
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(icar_hip_last_error(), msg, [512])
    n = 0
    do while (n < 512)
       if (msg(n+1) == c_null_char) exit
       n = n + 1
    end do
    write(*,*) "icar_hip: ", what, ": ", msg(1:n)
    error stop "icar_hip call failed"
  end subroutine

  !> one context per image; ims..jme are the tile's memory bounds (domain%grid%ims ...)
  subroutine hip_create(ctx, device, ims, ime, kms, kme, jms, jme)
    type(hip_ctx_t), intent(out) :: ctx
    integer, intent(in) :: device, ims, ime, kms, kme, jms, jme
    call check(icar_hip_ctx_create(ctx%p, int(device,c_int), int(ims,c_int), int(ime,c_int), int(kms,c_int), &
                                   int(kme,c_int), int(jms,c_int), int(jme,c_int)), "ctx_create")
  end subroutine

  subroutine hip_destroy(ctx)
    type(hip_ctx_t), intent(inout) :: ctx
    call check(icar_hip_ctx_destroy(ctx%p), "ctx_destroy"); ctx%p = c_null_ptr
  end subroutine

  subroutine hip_sync(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_synchronize(ctx%p), "synchronize")
  end subroutine

  !> make_winds_grid_relative(u, v, w, sintheta, costheta) of wind.f90:236-287 on the device u, v (update: their dqdt_3d);
  !! upload domain%sintheta / costheta with hip_upload_2dd(ctx, ICAR_F_SINTHETA / ICAR_F_COSTHETA, ...) once after init_winds
  subroutine hip_make_winds_grid_relative(ctx, update)
    type(hip_ctx_t), intent(in) :: ctx
    logical, intent(in) :: update
    call check(icar_hip_make_winds_grid_relative(ctx%p, merge(1_c_int,0_c_int,update)), "make_winds_grid_relative")
  end subroutine

  !> second HIP stream: `call hip_aux_fork(ctx)` before mp(halo=1); the interior mp(subset=1) between
  !! hip_aux_begin / hip_aux_end runs beside the strips + halo_send; hip_aux_join before halo_retrieve (time_step.f90:512-526)
  subroutine hip_aux_fork(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_aux_fork(ctx%p), "aux_fork")
  end subroutine
  subroutine hip_aux_begin(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_aux_begin(ctx%p), "aux_begin")
  end subroutine
  subroutine hip_aux_end(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_aux_end(ctx%p), "aux_end")
  end subroutine
  subroutine hip_aux_join(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_aux_join(ctx%p), "aux_join")
  end subroutine

  !> compute_dt's strictness-3 reduction left on the device (d_out = device address of one REAL(4)), for a device-side co_min
  subroutine hip_max_courant_device(ctx, dx, dz_levels, d_out)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx, dz_levels(:)
    type(c_ptr), intent(in) :: d_out
    call check(icar_hip_max_courant_device(ctx%p, real(dx,c_float), dz_levels, d_out), "max_courant_device")
  end subroutine

  !> domain%X%data_3d -> device.  The reference allocates these whole-array, i.e. contiguous; the
  !! pointers are not declared CONTIGUOUS (exchangeable_h.f90:14), so assert it before c_loc.
  subroutine hip_upload(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_float), intent(in), target, contiguous :: a(:,:,:)
    call check(icar_hip_field_upload(ctx%p, field, c_loc(a)), "field_upload")
  end subroutine

  subroutine hip_download(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_float), intent(inout), target, contiguous :: a(:,:,:)
    call check(icar_hip_field_download(ctx%p, field, c_loc(a)), "field_download")
  end subroutine

  subroutine hip_upload_2dd(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_double), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_field_upload(ctx%p, field, c_loc(a)), "field_upload")
  end subroutine

  subroutine hip_download_2dd(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_double), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_field_download(ctx%p, field, c_loc(a)), "field_download")
  end subroutine

  !> domain%terrain%data_2d (REAL(4)) and domain%land_mask (INTEGER) -> ICAR_F_TERRAIN / ICAR_F_LAND_MASK, what simple_pbl reads
  subroutine hip_upload_2d(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_float), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_field_upload(ctx%p, field, c_loc(a)), "field_upload")
  end subroutine

  subroutine hip_upload_2di(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    integer(c_int), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_field_upload(ctx%p, field, c_loc(a)), "field_upload")
  end subroutine

  !> advect(domain, options, dt) of advection_driver.f90:51 : scheme = options%physics%advection,
  !! vars = field ids with options%vars_to_advect(...)>0 in the order of adv_mpdata.f90:512-522.
  subroutine hip_advect(ctx, scheme, mpdata_order, fct, advect_density, dt, dx, vars)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: scheme, mpdata_order
    logical, intent(in) :: fct, advect_density
    real, intent(in) :: dt, dx
    integer(c_int), intent(in) :: vars(:)
    call check(icar_hip_setup_winds(ctx%p, int(scheme,c_int), real(dt,c_float), real(dx,c_float), &
                                    merge(1_c_int,0_c_int,advect_density)), "setup_winds")
    call check(icar_hip_advect(ctx%p, int(scheme,c_int), int(mpdata_order,c_int), merge(1_c_int,0_c_int,fct), &
                               merge(1_c_int,0_c_int,advect_density), vars, int(size(vars),c_int)), "advect")
  end subroutine

  !> mp_simple_driver (mp_simple.f90:595) on a tile, incl. the precipitation accumulation of process_subdomain
  subroutine hip_mp_simple(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_mp_simple(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                                  int(kts,c_int), int(kte,c_int), c_null_ptr), "mp_simple")
  end subroutine

  subroutine hip_thompson_init(ctx, params, Ef_rw_l, Ef_sw_l)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_float), intent(in) :: params(18)      ! mp_options_type in declaration order (opt_types.f90:30-41)
    logical, intent(in) :: Ef_rw_l, Ef_sw_l
    integer(c_int) :: flags(2)
    flags = [merge(1_c_int,0_c_int,Ef_rw_l), merge(1_c_int,0_c_int,Ef_sw_l)]
    call check(icar_hip_thompson_init(ctx%p, params, flags), "thompson_init")
  end subroutine

  subroutine hip_thompson(ctx, dt, its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte, ids, ide, jds, jde, kds, kde
    call check(icar_hip_thompson(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
               int(kts,c_int), int(kte,c_int), int(ids,c_int), int(ide,c_int), int(jds,c_int), int(jde,c_int), &
               int(kds,c_int), int(kde,c_int)), "thompson")
  end subroutine

  !> the reduction inside compute_dt (time_step.f90:264-289); dt = CFL / result
  real function hip_max_courant(ctx, dx, dz_levels)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    real(c_float), intent(in) :: dz_levels(:)
    real(c_float) :: r
    call check(icar_hip_max_courant(ctx%p, real(dx,c_float), dz_levels, r), "max_courant")
    hip_max_courant = r
  end function

  subroutine hip_balance_uvw(ctx, dx)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    call check(icar_hip_balance_uvw(ctx%p, real(dx,c_float)), "balance_uvw")
  end subroutine

  !> the CFL reduction of the NEXT update_dt taken now, on the current stream (beside the advection, after the forcing of u, v, w)
  subroutine hip_max_courant_prefetch(ctx, dx, dz_levels)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    real(c_float), intent(in) :: dz_levels(:)
    call check(icar_hip_max_courant_prefetch(ctx%p, real(dx,c_float), dz_levels), "max_courant_prefetch")
  end subroutine

  !> process_halo's strips for WSM6 in one sequence of launches: tiles(1:4, t) = its, ite, jts, jte of strip t
  subroutine hip_wsm6_tiles(ctx, dt, tiles, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer(c_int), intent(in) :: tiles(:,:)
    integer, intent(in) :: kts, kte
    call check(icar_hip_wsm6_tiles(ctx%p, real(dt,c_float), int(size(tiles,2),c_int), tiles, int(kts,c_int), int(kte,c_int)), "wsm6_tiles")
  end subroutine

  !> .true. while the Courant winds of the last hip_setup_winds still belong to the state
  logical function hip_winds_valid(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    hip_winds_valid = icar_hip_winds_valid(ctx%p) /= 0
  end function

  !> wsm6init / wsm6 as mp_driver.f90:100 and :518-550 call them
  subroutine hip_wsm6_init(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_wsm6_init(ctx%p), "wsm6_init")
  end subroutine

  subroutine hip_wsm6(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_wsm6(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                             int(kts,c_int), int(kte,c_int)), "wsm6")
  end subroutine

  !> wsm3init / wsm3 as mp_driver.f90:105 and :552-585 call them (qci = cloud_water_mass, qrs = rain_mass, w = w_real)
  subroutine hip_wsm3_init(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_wsm3_init(ctx%p), "wsm3_init")
  end subroutine

  subroutine hip_wsm3(ctx, dt, its, ite, jts, jte, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer, intent(in) :: its, ite, jts, jte, kts, kte
    call check(icar_hip_wsm3(ctx%p, real(dt,c_float), int(its,c_int), int(ite,c_int), int(jts,c_int), int(jte,c_int), &
                             int(kts,c_int), int(kte,c_int)), "wsm3")
  end subroutine

  !> diagnostic_update in parts: 1 = all but w_real, 2 = w_real only (can run beside the interior microphysics), 3 = both
  subroutine hip_diagnostic_update_parts(ctx, parts)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: parts
    call check(icar_hip_diagnostic_update_parts(ctx%p, int(parts,c_int)), "diagnostic_update_parts")
  end subroutine

  !> diagnostic_update (time_step.f90:49-198)
  subroutine hip_diagnostic_update(ctx)
    type(hip_ctx_t), intent(in) :: ctx
    call check(icar_hip_diagnostic_update(ctx%p), "diagnostic_update")
  end subroutine

  !> the look-up tables of forcing%geo / %geo_u / %geo_v, domain%nsmooth and, for adjust_pressure, forcing%geo%z with domain%geo%z:
  !! once, behind the reference's geo_LUT / vLUT (init time).  Every index is validated before anything is stored.
  subroutine hip_forcing_configure(ctx, mass, nsmooth, u, v, forcing_z, domain_z, time_varying_z)
    type(hip_ctx_t), intent(in) :: ctx
    type(hip_forcing_geo_t), intent(in), target :: mass
    integer, intent(in) :: nsmooth
    type(hip_forcing_geo_t), intent(in), target, optional :: u, v
    real(c_float), intent(in), target, contiguous, optional :: forcing_z(:,:,:), domain_z(:,:,:)
    logical, intent(in), optional :: time_varying_z
    type(forcing_geo_c), target :: cm, cu, cv
    type(c_ptr) :: pu, pv, pzf, pzd
    integer(c_int) :: tvz
    cm = as_c(mass); pu = c_null_ptr; pv = c_null_ptr; pzf = c_null_ptr; pzd = c_null_ptr; tvz = 0
    if (present(u)) then; cu = as_c(u); pu = c_loc(cu); endif
    if (present(v)) then; cv = as_c(v); pv = c_loc(cv); endif
    if (present(forcing_z)) pzf = c_loc(forcing_z)
    if (present(domain_z)) pzd = c_loc(domain_z)
    if (present(time_varying_z)) tvz = merge(1_c_int, 0_c_int, time_varying_z)
    call check(icar_hip_forcing_configure(ctx%p, c_loc(cm), pu, pv, int(nsmooth,c_int), pzf, pzd, tvz), "forcing_configure")
  contains
    function as_c(g) result(c)
      type(hip_forcing_geo_t), intent(in), target :: g
      type(forcing_geo_c) :: c
      c%x = c_loc(g%x); c%y = c_loc(g%y); c%w = c_loc(g%w); c%z = c_loc(g%z); c%zw = c_loc(g%zw)
      c%nx = int(size(g%x,2),c_int); c%ny = int(size(g%x,3),c_int)
      c%nx_f = int(g%nx_f,c_int); c%nz_f = int(g%nz_f,c_int); c%ny_f = int(g%ny_f,c_int); c%i0 = int(g%i0,c_int); c%j0 = int(g%j0,c_int)
    end function
  end subroutine

  !> input_data%data_3d of the forcing variable of `field`, as boundary%update_forcing has just read it
  subroutine hip_forcing_upload(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_float), intent(in), target, contiguous :: a(:,:,:)
    call check(icar_hip_forcing_upload(ctx%p, field, c_loc(a), int(size(a,1),c_int), int(size(a,2),c_int), int(size(a,3),c_int)), "forcing_upload")
  end subroutine

  !> domain%interpolate_forcing(forcing, update) (domain_obj.f90:2559-2643) over the listed 3-D fields; pressure_field < 0: none
  subroutine hip_interpolate_forcing(ctx, fields, pressure_field, theta_field, update)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: fields(:), pressure_field, theta_field
    logical, intent(in) :: update
    call check(icar_hip_interpolate_forcing(ctx%p, fields, int(size(fields),c_int), pressure_field, theta_field, merge(1_c_int, 0_c_int, update)), &
               "interpolate_forcing")
  end subroutine

  !> domain%update_delta_fields(dt) (domain_obj.f90:2339-2372); w is always included
  subroutine hip_update_delta_fields(ctx, fields, dt_seconds)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: fields(:)
    double precision, intent(in) :: dt_seconds
    call check(icar_hip_update_delta_fields(ctx%p, fields, int(size(fields),c_int), real(dt_seconds,c_double)), "update_delta_fields")
  end subroutine

  !> driver.f90:133-137 behind boundary%update_forcing: interpolate_forcing(update=.True.), update_winds, update_delta_fields
  subroutine hip_forcing_step(ctx, fields, pressure_field, theta_field, windtype, wind_iterations, dx, halo, dt_seconds)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: fields(:), pressure_field, theta_field
    integer, intent(in) :: windtype, wind_iterations, halo
    real, intent(in) :: dx
    double precision, intent(in) :: dt_seconds
    call check(icar_hip_forcing_step(ctx%p, fields, int(size(fields),c_int), pressure_field, theta_field, int(windtype,c_int), &
               int(wind_iterations,c_int), real(dx,c_float), int(halo,c_int), real(dt_seconds,c_double)), "forcing_step")
  end subroutine

  !> input_data%data_2d of a forced 2-D variable (ICAR_FORCED2D_*), as boundary%update_forcing has just read it
  subroutine hip_forcing2d_upload(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_forcing2d_upload(ctx%p, which, c_loc(a), int(size(a,1),c_int), int(size(a,2),c_int)), "forcing2d_upload")
  end subroutine

  subroutine hip_forcing2d_download(ctx, which, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which
    real(c_float), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_forcing2d_download(ctx%p, which, c_loc(a), int(size(a),c_size_t)), "forcing2d_download")
  end subroutine

  !> the two_d branch of domain%interpolate_forcing (domain_obj.f90:2595-2600): geo_interp2d into dqdt_2d (update) or data_2d
  subroutine hip_forcing2d_interpolate(ctx, which, update)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which(:)
    logical, intent(in) :: update
    call check(icar_hip_interpolate_forcing_2d(ctx%p, which, int(size(which),c_int), merge(1_c_int, 0_c_int, update)), "interpolate_forcing_2d")
  end subroutine

  !> domain%update_delta_fields(dt) for 2-D variables (domain_obj.f90:2355-2356)
  subroutine hip_forcing2d_update_delta(ctx, which, dt_seconds)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which(:)
    double precision, intent(in) :: dt_seconds
    call check(icar_hip_update_delta_fields_2d(ctx%p, which, int(size(which),c_int), real(dt_seconds,c_double)), "update_delta_fields_2d")
  end subroutine

  !> domain%apply_forcing(dt) for the enabled 2-D variables and the precipitation sum (domain_obj.f90:2400-2402, :2438-2445)
  subroutine hip_forcing2d_apply(ctx, dt_seconds)
    type(hip_ctx_t), intent(in) :: ctx
    double precision, intent(in) :: dt_seconds
    call check(icar_hip_apply_forcing_2d(ctx%p, real(dt_seconds,c_double)), "apply_forcing_2d")
  end subroutine

  !> the 2-D variables hip_forcing_step and every sub-step handle from now on; a zero-sized list disables
  subroutine hip_forcing2d_enable(ctx, which)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which(:)
    call check(icar_hip_forcing2d_enable(ctx%p, which, int(size(which),c_int)), "forcing2d_enable")
  end subroutine

  !> data_2d (ICAR_FORCED2D_DATA) or dqdt_2d (ICAR_FORCED2D_DQDT) of one forced 2-D variable, (nx, ny): restart files
  subroutine hip_forcing2d_get(ctx, which, what, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which, what
    real(c_float), intent(inout), target, contiguous :: a(:,:)
    call check(icar_hip_forcing2d_get(ctx%p, which, what, c_loc(a)), "forcing2d_get")
  end subroutine

  subroutine hip_forcing2d_set(ctx, which, what, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: which, what
    real(c_float), intent(in), target, contiguous :: a(:,:)
    call check(icar_hip_forcing2d_set(ctx%p, which, what, c_loc(a)), "forcing2d_set")
  end subroutine

  !> variable%meta_data%dqdt_3d -> device (the forcing tendency apply_forcing adds)
  subroutine hip_dqdt_upload(ctx, field, a)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: field
    real(c_float), intent(in), target, contiguous :: a(:,:,:)
    call check(icar_hip_dqdt_upload(ctx%p, field, c_loc(a)), "dqdt_upload")
  end subroutine

  !> domain%apply_forcing(dt) (domain_obj.f90:2383-2448): force_boundaries(i) -> only the true domain edges
  subroutine hip_apply_forcing(ctx, dt_seconds, fields, force_boundaries, west, east, south, north)
    type(hip_ctx_t), intent(in) :: ctx
    double precision, intent(in) :: dt_seconds
    integer(c_int), intent(in) :: fields(:)
    logical, intent(in) :: force_boundaries(:), west, east, south, north
    integer(c_int) :: fb(size(fields))
    fb = merge(1_c_int, 0_c_int, force_boundaries)
    call check(icar_hip_apply_forcing(ctx%p, real(dt_seconds,c_double), fields, fb, int(size(fields),c_int), &
               merge(1_c_int,0_c_int,west), merge(1_c_int,0_c_int,east), merge(1_c_int,0_c_int,south), merge(1_c_int,0_c_int,north)), &
               "apply_forcing")
  end subroutine

  !> domain%enforce_limits() (domain_obj.f90:2228-2243)
  subroutine hip_enforce_limits(ctx, fields)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: fields(:)
    call check(icar_hip_enforce_limits(ctx%p, fields, int(size(fields),c_int)), "enforce_limits")
  end subroutine

  !> halo faces of all exchanged scalars in one device buffer per neighbour (exchangeable_obj.f90:248-356).
  !! dir: 0 north, 1 south, 2 east, 3 west.  dbuf is a DEVICE pointer (hipMalloc / GPU-aware MPI window).
  integer(c_size_t) function hip_halo_count(ctx, dir, halo)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: dir, halo
    hip_halo_count = icar_hip_halo_count(ctx%p, int(dir,c_int), int(halo,c_int))
  end function

  subroutine hip_halo_pack(ctx, dir, halo, fields, dbuf)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: dir, halo
    integer(c_int), intent(in) :: fields(:)
    type(c_ptr), intent(in) :: dbuf
    call check(icar_hip_halo_pack(ctx%p, int(dir,c_int), int(halo,c_int), fields, int(size(fields),c_int), dbuf), "halo_pack")
  end subroutine

  subroutine hip_halo_unpack(ctx, dir, halo, fields, dbuf)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: dir, halo
    integer(c_int), intent(in) :: fields(:)
    type(c_ptr), intent(in) :: dbuf
    call check(icar_hip_halo_unpack(ctx%p, int(dir,c_int), int(halo,c_int), fields, int(size(fields),c_int), dbuf), "halo_unpack")
  end subroutine

  !> process_halo's strips for mp_simple in one launch: tiles(1:4, t) = its, ite, jts, jte of strip t
  subroutine hip_mp_simple_tiles(ctx, dt, tiles, kts, kte)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer(c_int), intent(in) :: tiles(:,:)
    integer, intent(in) :: kts, kte
    call check(icar_hip_mp_simple_tiles(ctx%p, real(dt,c_float), int(size(tiles,2),c_int), tiles, int(kts,c_int), int(kte,c_int), &
                                        c_null_ptr), "mp_simple_tiles")
  end subroutine

  !> every direction of one halo_send / halo_retrieve in one launch (dirs(t), dbufs(t))
  subroutine hip_halo_pack_dirs(ctx, dirs, halo, fields, dbufs)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: dirs(:), fields(:)
    integer, intent(in) :: halo
    type(c_ptr), intent(in) :: dbufs(:)
    call check(icar_hip_halo_pack_dirs(ctx%p, int(size(dirs),c_int), dirs, int(halo,c_int), fields, int(size(fields),c_int), dbufs), "halo_pack_dirs")
  end subroutine

  subroutine hip_halo_unpack_dirs(ctx, dirs, halo, fields, dbufs)
    type(hip_ctx_t), intent(in) :: ctx
    integer(c_int), intent(in) :: dirs(:), fields(:)
    integer, intent(in) :: halo
    type(c_ptr), intent(in) :: dbufs(:)
    call check(icar_hip_halo_unpack_dirs(ctx%p, int(size(dirs),c_int), dirs, int(halo,c_int), fields, int(size(fields),c_int), dbufs), "halo_unpack_dirs")
  end subroutine

  !> process_halo's strips (mp_driver.f90:609-658) in one launch: tiles(1:4, t) = its, ite, jts, jte of strip t
  subroutine hip_thompson_tiles(ctx, dt, tiles, kts, kte, ids, ide, jds, jde, kds, kde)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    integer(c_int), intent(in) :: tiles(:,:)
    integer, intent(in) :: kts, kte, ids, ide, jds, jde, kds, kde
    call check(icar_hip_thompson_tiles(ctx%p, real(dt,c_float), int(size(tiles,2),c_int), tiles, int(kts,c_int), int(kte,c_int), &
               int(ids,c_int), int(ide,c_int), int(jds,c_int), int(jde,c_int), int(kds,c_int), int(kde,c_int)), "thompson_tiles")
  end subroutine

  !> mass_conservative_acceleration (wind.f90:500-511) with ICAR_F_ZR_U / ICAR_F_ZR_V uploaded
  subroutine hip_mass_conservative_acceleration(ctx, update)
    type(hip_ctx_t), intent(in) :: ctx
    logical, intent(in) :: update
    call check(icar_hip_mass_conservative_acceleration(ctx%p, merge(1_c_int,0_c_int,update)), "mass_conservative_acceleration")
  end subroutine

  subroutine hip_balance_uvw_update(ctx, dx)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    call check(icar_hip_balance_uvw_update(ctx%p, real(dx,c_float)), "balance_uvw_update")
  end subroutine

  !> iterative_winds (wind.f90:371-498) on ONE image (exchange_u / exchange_v are no-ops there): balance_uvw, the model-top
  !> correction of w, then wind_iterations+1 Jacobi sweeps.  A multi-image host calls the two entry points itself and
  !> keeps its `call domain%u%exchange_u(); call domain%v%exchange_v()` between single sweeps.
  subroutine hip_iterative_winds(ctx, dx, wind_iterations, update)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    integer, intent(in) :: wind_iterations
    logical, intent(in), optional :: update
    integer(c_int) :: upd
    upd = 0
    if (present(update)) upd = merge(1, 0, update)
    if (upd == 1) then
       call check(icar_hip_balance_uvw_update(ctx%p, real(dx,c_float)), "balance_uvw_update")
    else
       call check(icar_hip_balance_uvw(ctx%p, real(dx,c_float)), "balance_uvw")
    end if
    call check(icar_hip_iterative_winds_correct_w(ctx%p, upd), "iterative_winds_correct_w")
    call check(icar_hip_iterative_winds_sweep(ctx%p, real(dx,c_float), int(wind_iterations+1,c_int), upd), "iterative_winds_sweep")
  end subroutine

  !> the two pieces of iterative_winds for a host that keeps the loop (and its exchange_u / exchange_v per sweep) in its own hands:
  !! the model-top correction of w (wind.f90:430-441) and nsweeps Jacobi sweeps (:455-481: calc_divergence, ADJ, the u / v faces)
  subroutine hip_iterative_winds_correct_w(ctx, update)
    type(hip_ctx_t), intent(in) :: ctx
    logical, intent(in) :: update
    call check(icar_hip_iterative_winds_correct_w(ctx%p, merge(1_c_int, 0_c_int, update)), "iterative_winds_correct_w")
  end subroutine
  subroutine hip_iterative_winds_sweep(ctx, dx, nsweeps, update)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dx
    integer, intent(in) :: nsweeps
    logical, intent(in) :: update
    call check(icar_hip_iterative_winds_sweep(ctx%p, real(dx,c_float), int(nsweeps,c_int), merge(1_c_int, 0_c_int, update)), "iterative_winds_sweep")
  end subroutine

  !> update_winds(domain, options) (wind.f90:289-369) as one call, on any number of images: make_winds_grid_relative ->
  !! linear_perturb (windtype 1, 5) -> mass_conservative_acceleration (2) -> iterative_winds with its exchange_u / exchange_v
  !! per sweep (3, 5) -> balance_uvw.  The first call of a context works on u, v, w, later ones on their dqdt_3d, like the
  !! reference (`update` forces either).  windtype = options%physics%windtype, halo = grid%halo_size.
  subroutine hip_update_winds(ctx, windtype, wind_iterations, dx, halo, update)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: windtype, wind_iterations, halo
    real, intent(in) :: dx
    logical, intent(in), optional :: update
    integer(c_int) :: upd
    upd = -1
    if (present(update)) upd = merge(1, 0, update)
    call check(icar_hip_update_winds(ctx%p, int(windtype,c_int), int(wind_iterations,c_int), real(dx,c_float), int(halo,c_int), upd), "update_winds")
  end subroutine

  !> call domain%u%exchange_u(); call domain%v%exchange_v() (exchangeable_obj.f90:158-229), one message per neighbour
  subroutine hip_exchange_uv(ctx, halo, update)
    type(hip_ctx_t), intent(in) :: ctx
    integer, intent(in) :: halo
    logical, intent(in), optional :: update
    integer(c_int) :: upd
    upd = 0
    if (present(update)) upd = merge(1, 0, update)
    call check(icar_hip_exchange_uv(ctx%p, int(halo,c_int), upd), "exchange_uv")
  end subroutine

  !> setup_linwinds (linear_winds.f90:1180): terrain spectrum, wavenumber axes, zeroed perturbation state
  subroutine hip_setup_linwinds(ctx, lt, global_terrain, ids, jds, dx)
    type(hip_ctx_t), intent(in) :: ctx
    type(hip_lt_options_t), intent(in) :: lt
    real(c_float), contiguous, intent(in) :: global_terrain(:,:)
    integer, intent(in) :: ids, jds
    real, intent(in) :: dx
    call check(icar_hip_linwinds_setup(ctx%p, lt, global_terrain, int(size(global_terrain,1),c_int), &
               int(size(global_terrain,2),c_int), int(ids,c_int), int(jds,c_int), real(dx,c_float)), "linwinds_setup")
  end subroutine

  !> initialize_spatial_winds (linear_winds.f90:596), constant-z layers: z_bottom/top = layer_height -/+ dz_levels/2
  subroutine hip_linwinds_build_lut(ctx, z_bottom, z_top)
    type(hip_ctx_t), intent(in) :: ctx
    real(c_float), intent(in) :: z_bottom(:), z_top(:)
    call check(icar_hip_linwinds_build_lut(ctx%p, z_bottom, z_top, int(size(z_bottom),c_int)), "linwinds_build_lut")
  end subroutine

  !> spatial_winds (linear_winds.f90:840): update=.true. targets u/v dqdt_3d
  subroutine hip_spatial_winds(ctx, update)
    type(hip_ctx_t), intent(in) :: ctx
    logical, intent(in) :: update
    call check(icar_hip_spatial_winds(ctx%p, merge(1_c_int, 0_c_int, update)), "spatial_winds")
  end subroutine
end module icar_hip

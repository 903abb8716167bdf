! tests/support/ysu_glue.f90 -- TEST INFRASTRUCTURE, compile-only: a caller of the YSU bindings of icar_amd/fortran/icar_hip_mod.f90 as
! INTEGRATION.md section 3 ("YSU") shows them, with the ranks and kinds a host's domain_t members have (REAL(4) 2-D and 3-D arrays, an
! INTEGER 2-D kpbl).  tests/test_ysu_fortran_compiles.py compiles it against the module; it is never run.
subroutine ysu_glue(hip, boundarylayer, dt, its, ite, jts, jte, kts, kte, ground_surf_temperature, hpbl, exch_h, tend_th, kpbl)
  use icar_hip
  implicit none
  type(hip_ctx_t), intent(in) :: hip
  integer, intent(in) :: boundarylayer, its, ite, jts, jte, kts, kte
  real, intent(in) :: dt
  real, intent(inout), target, contiguous :: ground_surf_temperature(:,:), hpbl(:,:), exch_h(:,:,:), tend_th(:,:,:)
  integer, intent(inout), target, contiguous :: kpbl(:,:)
  call hip_pbl_init(hip, boundarylayer)
  call hip_ysu_upload(hip, ICAR_YSU_GROUND_SURF_TEMPERATURE, ground_surf_temperature)
  if (boundarylayer == ICAR_PBL_YSU) call hip_pbl(hip, dt)
  call hip_ysu_sfc(hip)
  call hip_ysu(hip, dt, its,ite, jts,jte, kts,kte)
  call hip_ysu_download(hip, ICAR_YSU_HPBL, hpbl)
  call hip_ysu_download(hip, ICAR_YSU_EXCH_H, exch_h)
  call hip_ysu_download(hip, ICAR_YSU_TEND_TH, tend_th)
  call hip_ysu_upload(hip, ICAR_YSU_TEND_TH, tend_th)
  call hip_ysu_download_kpbl(hip, kpbl)
end subroutine

! tests/support/integration_glue_lsm_noah.f90 -- TEST INFRASTRUCTURE (compiled with -fsyntax-only by tests/test_lsm_noah_driver_abi.py): what
! a host's lsm_init and lsm do once the Noah branch of lsm() runs on the device (INTEGRATION.md, section 3).  The host keeps no statement
! of lsm_driver.f90:1028-1546 and uploads neither CHS, Ri, QGH nor current_precipitation.
module lsm_noah_glue
  use icar_hip
  implicit none
contains
  !> behind the host's own lsm_init for Noah (hip_noah_tables, the hip_noah_upload calls and hip_lsm_init have run): lsm_driver.f90:566,
  !! :583-611, :992-997 on the device
  subroutine glue_lsm_init(ctx, roughness_z0, accumulated_precipitation)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: roughness_z0(:,:)
    double precision, intent(in) :: accumulated_precipitation(:,:)
    call hip_upload_2d(ctx, ICAR_F_ROUGHNESS_Z0, roughness_z0)
    call hip_upload_2dd(ctx, ICAR_F_PRECIPITATION, accumulated_precipitation)
    call hip_lsm_noah_couple(ctx)
  end subroutine

  !> lsm(domain, options, dt) at time_step.f90:491 when the host drives the slots itself; hip_step / hip_step_n run it inside the step
  subroutine glue_lsm(ctx, dt)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: dt
    call hip_lsm(ctx, dt)
  end subroutine

  !> what an output step or a restart file reads
  subroutine glue_lsm_output(ctx, temperature_2m, humidity_2m, longwave_up, rainbl, soil_totalmoisture)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(inout) :: temperature_2m(:,:), humidity_2m(:,:), longwave_up(:,:), soil_totalmoisture(:,:)
    double precision, intent(inout) :: rainbl(:,:)
    call hip_lsm_download(ctx, ICAR_LSM_TEMPERATURE_2M, temperature_2m)
    call hip_lsm_download(ctx, ICAR_LSM_HUMIDITY_2M, humidity_2m)
    call hip_lsm_download(ctx, ICAR_LSM_LONGWAVE_UP, longwave_up)
    call hip_lsm_download_r8(ctx, ICAR_LSM_RAINBL, rainbl)
    call hip_noah_download(ctx, ICAR_NOAH_SOIL_TOTALMOISTURE, soil_totalmoisture)
  end subroutine

  !> a restart: behind hip_lsm_init and hip_lsm_noah_couple, the arrays of the run that wrote the file
  subroutine glue_lsm_restart(ctx, temperature_2m, humidity_2m, rainbl)
    type(hip_ctx_t), intent(in) :: ctx
    real, intent(in) :: temperature_2m(:,:), humidity_2m(:,:)
    double precision, intent(in) :: rainbl(:,:)
    call hip_lsm_upload(ctx, ICAR_LSM_TEMPERATURE_2M, temperature_2m)
    call hip_lsm_upload(ctx, ICAR_LSM_HUMIDITY_2M, humidity_2m)
    call hip_lsm_upload_r8(ctx, ICAR_LSM_RAINBL, rainbl)
  end subroutine
end module

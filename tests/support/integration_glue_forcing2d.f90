!> tests/support/integration_glue_forcing2d.f90 -- TEST INFRASTRUCTURE (build container only; nothing of this travels to the GPU box).
!! The statements of INTEGRATION.md's block for the 2-D forced variables (section 2, fenced as f95), verbatim, inside a subroutine whose
!! dummies are the REFERENCE's own domain_t / variable_t / time_delta_t next to `use icar_hip`:
!! tests/test_forcing2d_integration_compiles.py runs flang -fsyntax-only on it, so a member that INTEGRATION.md names and the reference
!! does not have, or an argument of the wrong type / kind / rank, is a compile error here.  Same scheme as
!! tests/support/integration_glue_forcing.f90.
module integration_glue_forcing2d
  use, intrinsic :: iso_c_binding
  use domain_interface,   only : domain_t
  use variable_interface, only : variable_t
  use time_delta_object,  only : time_delta_t
  use icar_hip
  implicit none
contains

  !> main/driver.f90:132-137, main/init.f90 get_initial_conditions, main/driver.f90:179,190
  subroutine glue_forcing2d(domain, hip, input_data, dt)
    type(domain_t), intent(inout) :: domain
    type(hip_ctx_t), intent(in) :: hip                                    ! (INTEGRATION: a member of domain_t, domain%hip)
    type(variable_t), intent(in) :: input_data
    type(time_delta_t), intent(in) :: dt
    integer(c_int) :: forced_2d(4)
    call hip_forcing2d_upload(hip, ICAR_FORCED2D_SST, input_data%data_2d)
    forced_2d = [ICAR_FORCED2D_SST, ICAR_FORCED2D_SHORTWAVE, ICAR_FORCED2D_LONGWAVE, ICAR_FORCED2D_EXTERNAL_PRECIPITATION]
    call hip_forcing2d_interpolate(hip, forced_2d, update=.false.)
    call hip_forcing2d_enable(hip, forced_2d)
    call hip_forcing2d_interpolate(hip, forced_2d, update=.true.)
    call hip_forcing2d_update_delta(hip, forced_2d, dt%seconds())
    call hip_forcing2d_apply(hip, dt%seconds())
    call hip_forcing2d_get(hip, ICAR_FORCED2D_EXTERNAL_PRECIPITATION, ICAR_FORCED2D_DATA, domain%external_precipitation%data_2d)
    call hip_forcing2d_get(hip, ICAR_FORCED2D_SST, ICAR_FORCED2D_DQDT, domain%sst%dqdt_2d)
    call hip_forcing2d_set(hip, ICAR_FORCED2D_SST, ICAR_FORCED2D_DQDT, domain%sst%dqdt_2d)
  end subroutine
end module

!> tests/support/integration_glue_forcing.f90 -- TEST INFRASTRUCTURE (build container only; nothing of this travels to the GPU box).
!! The statements of INTEGRATION.md's forcing block (section 2, fenced as f90), verbatim, inside a subroutine whose dummies are the
!! REFERENCE's own domain_t / boundary_t / options_t / variable_t / time_delta_t (the module files oracle/build_ref.sh compiles from the
!! reference's src/objects, unmodified) next to `use icar_hip`: tests/test_forcing_integration_compiles.py runs flang -fsyntax-only on it,
!! so a member that INTEGRATION.md names and the reference does not have, or an argument of the wrong type / kind / rank, is a compile
!! error here.  Same scheme as tests/support/integration_glue.f90, which holds the `fortran` blocks.
module integration_glue_forcing
  use, intrinsic :: iso_c_binding
  use domain_interface,   only : domain_t
  use options_interface,  only : options_t
  use boundary_interface, only : boundary_t
  use variable_interface, only : variable_t
  use time_delta_object,  only : time_delta_t
  use icar_hip
  implicit none
contains

  !> objects/domain_obj.f90 behind setup_geo_interpolation; main/driver.f90:132-137
  subroutine glue_forcing(this, domain, forcing, options, hip, input_data, forced_fields, dt)
    type(domain_t), intent(inout) :: this, domain
    type(boundary_t), intent(inout), target :: forcing
    type(options_t), intent(in) :: options
    type(hip_ctx_t), intent(in) :: hip                                    ! (INTEGRATION: a member of domain_t, this%hip)
    type(variable_t), intent(in) :: input_data
    integer(c_int), intent(in) :: forced_fields(:)
    type(time_delta_t), intent(in) :: dt
    type(hip_forcing_geo_t) :: gm, gu, gv
    gm%x => forcing%geo%geolut%x; gm%y => forcing%geo%geolut%y; gm%w => forcing%geo%geolut%w
    gm%z => forcing%geo%vert_lut%z; gm%zw => forcing%geo%vert_lut%w
    gm%nx_f = size(forcing%geo%lat,1); gm%nz_f = size(forcing%geo%z,2); gm%ny_f = size(forcing%geo%lat,2)
    gu%x => forcing%geo_u%geolut%x; gu%y => forcing%geo_u%geolut%y; gu%w => forcing%geo_u%geolut%w
    gu%z => forcing%geo_u%vert_lut%z; gu%zw => forcing%geo_u%vert_lut%w
    gu%nx_f = size(forcing%geo_u%lat,1); gu%nz_f = size(forcing%geo_u%z,2); gu%ny_f = size(forcing%geo_u%lat,2)
    gu%i0 = this%u_grid%ims - this%u_grid2d_ext%ims; gu%j0 = this%u_grid%jms - this%u_grid2d_ext%jms
    gv%x => forcing%geo_v%geolut%x; gv%y => forcing%geo_v%geolut%y; gv%w => forcing%geo_v%geolut%w
    gv%z => forcing%geo_v%vert_lut%z; gv%zw => forcing%geo_v%vert_lut%w
    gv%nx_f = size(forcing%geo_v%lat,1); gv%nz_f = size(forcing%geo_v%z,2); gv%ny_f = size(forcing%geo_v%lat,2)
    gv%i0 = this%v_grid%ims - this%v_grid2d_ext%ims; gv%j0 = this%v_grid%jms - this%v_grid2d_ext%jms
    call hip_forcing_configure(hip, gm, this%nsmooth, u=gu, v=gv, forcing_z=forcing%geo%z, domain_z=this%geo%z)
    call hip_forcing_upload(hip, ICAR_F_WATER_VAPOR, input_data%data_3d)
    call hip_forcing_step(hip, forced_fields, ICAR_F_PRESSURE, ICAR_F_POTENTIAL_TEMPERATURE, options%physics%windtype, &
                          options%parameters%wind_iterations, domain%dx, domain%grid%halo_size, dt%seconds())
    call hip_interpolate_forcing(hip, forced_fields, ICAR_F_PRESSURE, ICAR_F_POTENTIAL_TEMPERATURE, update=.true.)
    call hip_update_winds(hip, options%physics%windtype, options%parameters%wind_iterations, domain%dx, domain%grid%halo_size, update=.true.)
    call hip_update_delta_fields(hip, forced_fields, dt%seconds())
  end subroutine
end module

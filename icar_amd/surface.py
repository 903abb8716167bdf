"""land-surface driver mirror (src/physics/lsm_driver.f90): lsm_var_request / lsm_init / lsm, plus the parts on their own --
the 10 m diagnostics of diagnostic_update, water_simple and apply_fluxes.

Only landsurface = kLSM_BASIC (fluxes prescribed by the host or the forcing and applied to the atmosphere) with watersurface 0,
kWATER_BASIC (nothing runs) or kWATER_SIMPLE (src/physics/water_simple.f90: bulk fluxes over open water) is built; kLSM_SIMPLE stops
in the reference's own lsm_init and is refused with its message, Noah, Noah-MP and the lake model are refused by the library."""
import ctypes
from .capi import lib, check
from .constants import kLSM_BASIC, kWATER_SIMPLE


def lsm_var_request(options):
    """lsm_driver.f90:104-242: with kLSM_BASIC the reference requests nothing of its own (its blocks are those of kLSM_SIMPLE, Noah,
    Noah-MP and the lake model); what this path reads -- the fluxes, sst, roughness_z0, the 10 m winds, dz_interface -- the host
    uploads, which is the reference's `associated`.  kWATER_SIMPLE has no request either (water_simple.f90 has none)."""
    return


def lsm_configure(domain, landsurface, watersurface=0, update_interval=300, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0,
                  sfc_layer_thickness=400.0):
    """icar_hip_lsm_configure: the options of lsm_init; resets lsm's update gate and apply_fluxes' nz."""
    check(lib().icar_hip_lsm_configure(domain.ctx, int(landsurface), int(watersurface), int(update_interval), float(sh_feedback_fraction),
                                       float(lh_feedback_fraction), float(sfc_layer_thickness)), "icar_hip_lsm_configure")
    domain._lsm_key = ((int(landsurface), int(watersurface)) if int(landsurface) == 0 else
                       (int(landsurface), int(watersurface), int(update_interval), float(sh_feedback_fraction), float(lh_feedback_fraction), float(sfc_layer_thickness)))


def lsm_init(domain, options):
    """lsm_init (lsm_driver.f90:522-611, :991-1000): options%physics%landsurface / %watersurface and options%lsm_options to the library;
    QSFC = water_vapor(:,kms,:) when water_vapor is on the device."""
    o = options.lsm_options
    lsm_configure(domain, options.physics.landsurface, options.physics.watersurface, o.update_interval, o.sh_feedback_fraction,
                  o.lh_feedback_fraction, o.sfc_layer_thickness)


def lsm(domain, options, dt):
    """lsm(domain, options, dt) (lsm_driver.f90:1005-1554) on the tile its..kte of the domain's grid at the model clock: the update
    gate, water_simple inside it, apply_fluxes every call; dt a REAL(4) like real(dt%seconds())."""
    if options.physics.landsurface == 0:
        return
    domain.configure(options)
    check(lib().icar_hip_lsm(domain.ctx, float(dt)), "icar_hip_lsm")


def diag_10m(domain):
    """u_10m, v_10m and ustar of diagnostic_update (time_step.f90:143-161) from roughness_z0 and the mass-point winds"""
    check(lib().icar_hip_diag_10m(domain.ctx), "icar_hip_diag_10m")


def water_simple(domain):
    """windspd, its zero replacement and water_simple (lsm_driver.f90:1028-1073) on the memory interior"""
    check(lib().icar_hip_water_simple(domain.ctx), "icar_hip_water_simple")


def apply_fluxes(domain, dt, its, ite, jts, jte, kts, kte):
    """apply_fluxes(domain, dt) (lsm_driver.f90:361-423) on an explicit tile"""
    check(lib().icar_hip_apply_fluxes(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte), int(kts), int(kte)), "icar_hip_apply_fluxes")


def lsm_layers(domain, options):
    """apply_fluxes' nz for the grid's kts..kte: the last level below sfc_layer_thickness in the running sum of the levels' largest
    dz_interface over this image's memory (0: the first level is already thicker)"""
    domain.configure(options)
    n = ctypes.c_int()
    check(lib().icar_hip_lsm_layers(domain.ctx, ctypes.byref(n)), "icar_hip_lsm_layers")
    return n.value


def lsm_finalize(options, domain=None):
    """the slot is switched off"""
    if domain is not None:
        lsm_configure(domain, 0, 0)

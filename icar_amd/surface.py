"""land-surface driver mirror (src/physics/lsm_driver.f90): lsm_var_request / lsm_init / lsm, plus the parts on their own --
the 10 m diagnostics of diagnostic_update, water_simple and apply_fluxes.

landsurface = kLSM_BASIC (fluxes prescribed by the host or the forcing and applied to the atmosphere) with watersurface 0,
kWATER_BASIC (nothing runs) or kWATER_SIMPLE (src/physics/water_simple.f90: bulk fluxes over open water) is built whole; kLSM_SIMPLE stops
in the reference's own lsm_init and is refused with its message, Noah-MP and the lake model are refused by the library.  Of
kLSM_NOAH lsm_init's part and the call of lsm_noah are built (noah_tables, noah_init, lsm_noah, noah_set / noah_get); the rest of the
Noah branch of lsm() runs once noah_couple has been called behind noah_init (lsm_set / lsm_get hold its arrays); without that call
lsm() says that Noah runs through lsm_noah only."""
import ctypes

import numpy as np

from .capi import lib, check, noah_tables_c, noah_options_c, NOAH_T_VEG, NOAH_T_SOIL, NOAH_T_GEN, NOAH_T_INT
from .constants import kLSM_BASIC, kLSM_NOAH, kWATER_SIMPLE

# enum icar_hip_noah_array (include/icar_hip.h)
NOAH_ARRAYS = ["veg_type", "soil_type", "vegfrac", "soil_deep_temperature", "shdmin", "shdmax", "snoalb", "qgh", "chs", "cqs2", "ri",
               "current_precipitation", "ground_heat_flux", "smstav", "soil_totalmoisture", "sfcrunoff", "udrunoff", "albedo", "albbck", "z0", "emiss",
               "snowc", "snow_water_equivalent", "snow_height", "canopy_water", "chs2", "chklowq", "lai", "snotime", "acsnom", "acsnow", "snopcx",
               "potevp", "noahres", "flx4", "fvb", "fbur", "fgsn", "soil_water_content", "soil_temperature", "sh2o", "smcrel"]
NOAH_ID = {n: i for i, n in enumerate(NOAH_ARRAYS)}
NOAH_SOIL_LAYERS = 4
# enum icar_hip_lsm_array (include/icar_hip.h): (ny, nx) REAL(4), rainbl REAL(8)
LSM_ARRAYS = ["temperature_2m", "humidity_2m", "longwave_up", "rainbl", "z_atm", "lnz_atm_term", "base_exchange_term"]
LSM_ID = {n: i for i, n in enumerate(LSM_ARRAYS)}


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
    if options.physics.landsurface == kLSM_NOAH:
        return noah_init(domain, options)
    lsm_configure(domain, options.physics.landsurface, options.physics.watersurface, o.update_interval, o.sh_feedback_fraction,
                  o.lh_feedback_fraction, o.sfc_layer_thickness)


def noah_tables(domain, tab):
    """icar_hip_noah_tables: the tables as SOIL_VEG_GEN_PARM parsed them -- tab maps module_sf_noahlsm's variable names (lower case) to
    arrays of the module's extents and scalars"""
    t, keep = noah_tables_c(), []
    for n, dt_ in [("nrotbl", np.int32)] + [(n, np.float32) for n in NOAH_T_VEG + NOAH_T_SOIL + ["slope_data"]]:
        a = np.ascontiguousarray(tab[n], dt_); keep.append(a)
        setattr(t, n, a.ctypes.data)
    for n in NOAH_T_GEN: setattr(t, n, float(tab[n]))
    for n in NOAH_T_INT: setattr(t, n, int(tab[n]))
    check(lib().icar_hip_noah_tables(domain.ctx, ctypes.byref(t)), "icar_hip_noah_tables")


def _noah_shape(domain, name):
    return (domain.ny, NOAH_SOIL_LAYERS, domain.nx) if NOAH_ID[name] >= NOAH_ID["soil_water_content"] else (domain.ny, domain.nx)


def noah_set(domain, name, values):
    """icar_hip_noah_upload: one of NOAH_ARRAYS, (ny, nx) -- veg_type / soil_type INTEGER(4) -- or (ny, 4, nx) for the soil arrays"""
    a = np.ascontiguousarray(values, np.int32 if name in ("veg_type", "soil_type") else np.float32)
    if a.shape != _noah_shape(domain, name):
        raise ValueError(f"noah_set {name}: shape {a.shape}, expected {_noah_shape(domain, name)}")
    check(lib().icar_hip_noah_upload(domain.ctx, NOAH_ID[name], a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_noah_upload {name}")


def noah_get(domain, name):
    a = np.empty(_noah_shape(domain, name), np.int32 if name in ("veg_type", "soil_type") else np.float32)
    check(lib().icar_hip_noah_download(domain.ctx, NOAH_ID[name], a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_noah_download {name}")
    return a


def noah_init(domain, options, fndsnowh=False):
    """icar_hip_lsm_init: lsm_init with every landsurface that is built.  For kLSM_NOAH the tables (noah_tables) and the domain's
    arrays (noah_set: veg_type, soil_type, vegfrac, albedo, soil_deep_temperature, soil_water_content, soil_temperature) come first."""
    o, p = options.lsm_options, options.physics
    n = noah_options_c(int(o.urban_category), int(o.ice_category), int(o.water_category), int(o.lake_category), int(bool(o.monthly_vegfrac)),
                       int(bool(o.monthly_albedo)), int(bool(fndsnowh)), float(o.max_swe))
    check(lib().icar_hip_lsm_init(domain.ctx, int(p.landsurface), int(p.watersurface), int(o.update_interval), float(o.sh_feedback_fraction),
                                  float(o.lh_feedback_fraction), float(o.sfc_layer_thickness), ctypes.byref(n)), "icar_hip_lsm_init")
    domain._lsm_key = ((int(p.landsurface), int(p.watersurface)) if int(p.landsurface) == 0 else
                       (int(p.landsurface), int(p.watersurface), int(o.update_interval), float(o.sh_feedback_fraction), float(o.lh_feedback_fraction),
                        float(o.sfc_layer_thickness)))


def lsm_noah(domain, lsm_dt, its, ite, jts, jte):
    """icar_hip_lsm_noah: the call of lsm_noah (lsm_driver.f90:1210-1278) alone on a tile"""
    check(lib().icar_hip_lsm_noah(domain.ctx, float(lsm_dt), int(its), int(ite), int(jts), int(jte)), "icar_hip_lsm_noah")


def noah_couple(domain):
    """icar_hip_lsm_noah_couple: the rest of lsm_init for Noah (lsm_driver.f90:566, :583-611, :992-997), after noah_init; from here on
    lsm() and the step run the Noah branch of lsm() on the device"""
    check(lib().icar_hip_lsm_noah_couple(domain.ctx), "icar_hip_lsm_noah_couple")


def lsm_set(domain, name, values):
    """icar_hip_lsm_upload: one of LSM_ARRAYS, (ny, nx)"""
    a = np.ascontiguousarray(values, np.float64 if name == "rainbl" else np.float32)
    if a.shape != (domain.ny, domain.nx):
        raise ValueError(f"lsm_set {name}: shape {a.shape}, expected {(domain.ny, domain.nx)}")
    check(lib().icar_hip_lsm_upload(domain.ctx, LSM_ID[name], a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_lsm_upload {name}")


def lsm_get(domain, name):
    a = np.empty((domain.ny, domain.nx), np.float64 if name == "rainbl" else np.float32)
    check(lib().icar_hip_lsm_download(domain.ctx, LSM_ID[name], a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_lsm_download {name}")
    return a


def lsm(domain, options, dt):
    """lsm(domain, options, dt) (lsm_driver.f90:1005-1554) on the tile its..kte of the domain's grid at the model clock: the update
    gate, water_simple inside it (and, with Noah coupled by noah_couple, the whole Noah branch), apply_fluxes every call; dt a REAL(4)
    like real(dt%seconds())."""
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

"""boundary-layer driver mirror (src/physics/pbl_driver.f90): pbl_var_request / pbl_init / pbl / pbl_finalize.

Built: the simple scheme (kPBL_SIMPLE, src/physics/pbl_simple.f90, Hong and Pan 1996) and YSU (kPBL_YSU, src/physics/pbl_ysu.f90 with
da_sfc_wtq of src/utilities/pbl_utilities.f90, Hong, Noh and Dudhia 2006); kPBL_BASIC has no branch in the reference's driver either.
YSU's own arrays (hpbl, kpbl, exch_h, psim, ..., the six tendencies, the input ground_surf_temperature) have no field id: ysu_get /
ysu_set move them by the ICAR_YSU_* names below."""
import ctypes
import numpy as np
from .capi import lib, check
from .constants import kPBL_SIMPLE, kPBL_YSU

# enum icar_hip_ysu_array (include/icar_hip.h)
YSU_NAMES = {n: i for i, n in enumerate(["ground_surf_temperature", "hpbl", "kpbl", "exch_h", "psim", "psih", "regime", "ri", "windspd", "hol", "zol",
                                         "gz1oz0", "z_atm", "tend_th", "tend_qv", "tend_qc", "tend_qi", "tend_u", "tend_v"])}
YSU_3D = ("exch_h", "tend_th", "tend_qv", "tend_qc", "tend_qi", "tend_u", "tend_v")


YSU_VARS = ["water_vapor", "potential_temperature", "temperature", "exner", "dz_interface", "density", "pressure_interface", "skin_temperature",
            "terrain", "ground_surf_temperature", "sensible_heat", "latent_heat", "u_10m", "v_10m", "humidity_2m", "surface_pressure",
            "ground_heat_flux", "znu", "znw", "roughness_z0", "ustar", "cloud_ice", "tend_th_pbl", "tend_qc_pbl", "tend_qi_pbl", "temperature_2m",
            "tend_u", "tend_v", "tend_qv_pbl", "pressure", "kpbl", "land_mask", "cloud_water", "coeff_heat_exchange_3d", "hpbl"]


def pbl_var_request(options):
    """pbl_driver.f90:58-103, as written: the kPBL_SIMPLE block tests options%physics%landsurface (:62), not boundarylayer, so with
    the usual options (land surface off, or any scheme but number 2) choosing the simple PBL requests NOTHING -- the six scalars,
    exner, density, u and v it reads are there because the microphysics and the advection asked for them.  Reproduced, not
    repaired.  (dz_interface, u, v and land_mask are requested for allocation and restart by name; only the first two of the
    list are advected.)  The kPBL_YSU block (:76-102) tests boundarylayer: its list is allocated and written to restart files, four
    scalars are advected."""
    if options.physics.landsurface == kPBL_SIMPLE:
        options.alloc_vars(["water_vapor", "potential_temperature", "cloud_water", "cloud_ice", "rain_in_air", "snow_in_air",
                            "exner", "dz_interface", "density", "u", "v", "land_mask"])
        options.advect_vars(["potential_temperature", "water_vapor"])
        options.restart_vars(["water_vapor", "potential_temperature", "exner", "dz_interface", "density", "u", "v", "land_mask"])
    elif options.physics.boundarylayer == kPBL_YSU:
        options.alloc_vars(YSU_VARS)
        options.advect_vars(["potential_temperature", "water_vapor", "cloud_ice", "cloud_water"])
        options.restart_vars(YSU_VARS)


def pbl_init(domain, options):
    """pbl_driver.f90:106-195 (icar_hip_pbl_init): hands options%physics%boundarylayer to the library.  kPBL_SIMPLE: init_simple_pbl
    (pbl_simple.f90:296-330 allocates the module's work arrays; here the context allocates its own on the first call).  kPBL_YSU: the
    YSU branch :127-194 from the domain's z, terrain, roughness_z0 and land_mask, which must be on the device (IcarHipError names the
    missing member): z_atm, gz1oz0, zol, hol, the tendencies zeroed, the column workspace."""
    check(lib().icar_hip_pbl_init(domain.ctx, int(options.physics.boundarylayer)), "icar_hip_pbl_init")
    domain._pbl_key = int(options.physics.boundarylayer)


def pbl(domain, options, dt):
    """pbl(domain, options, dt_in) (pbl_driver.f90:197-354) on the tile its..kte of the domain's grid, dt a REAL(4) like
    real(dt%seconds()).  kPBL_SIMPLE: the six scalars, u_mass, v_mass, exner, density, z, dz_mass and terrain must be on the device
    (IcarHipError names the missing member); without a land_mask every cell is land.  kPBL_YSU: pbl_init must have run."""
    if options.physics.boundarylayer not in (kPBL_SIMPLE, kPBL_YSU):
        return
    domain.configure(options)
    check(lib().icar_hip_pbl(domain.ctx, float(dt)), "icar_hip_pbl")


def ysu_sfc(domain, options):
    """pbl_driver.f90:227-254 alone (icar_hip_ysu_sfc): windspd, Ri and da_sfc_wtq's psim, psih, regime over the whole memory"""
    domain.configure(options)
    check(lib().icar_hip_ysu_sfc(domain.ctx), "icar_hip_ysu_sfc")


def ysu(domain, dt, its, ite, jts, jte, kts, kte):
    """`call ysu(...)` alone (pbl_driver.f90:257-323) on an explicit tile; kte is the model's (the library lowers it by one as the
    driver does); the six tendencies stay where ysu leaves them"""
    check(lib().icar_hip_ysu(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte), int(kts), int(kte)), "icar_hip_ysu")


def _ysu_array(domain, name):
    which = YSU_NAMES[name] if isinstance(name, str) else int(name)
    name = [k for k, v in YSU_NAMES.items() if v == which][0]
    shape = (domain.ny, domain.nz, domain.nx) if name in YSU_3D else (domain.ny, domain.nx)
    return which, shape, np.int32 if name == "kpbl" else np.float32


def ysu_set(domain, name, array):
    which, shape, dtype = _ysu_array(domain, name)
    a = np.ascontiguousarray(array, dtype)
    if a.shape != shape:
        raise ValueError(f"{name}: shape {a.shape} != {shape}")
    check(lib().icar_hip_ysu_upload(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p), a.size), f"icar_hip_ysu_upload {name}")


def ysu_get(domain, name):
    which, shape, dtype = _ysu_array(domain, name)
    a = np.empty(shape, dtype)
    check(lib().icar_hip_ysu_download(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p), a.size), f"icar_hip_ysu_download {name}")
    return a


def simple_pbl(domain, dt, its, ite, jts, jte, kts, kte):
    """simple_pbl(...) (pbl_simple.f90:69-141) on an explicit tile of the domain's fields (icar_hip_pbl_simple)."""
    check(lib().icar_hip_pbl_simple(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte), int(kts), int(kte)), "icar_hip_pbl_simple")


def nsubsteps(domain):
    """the explicit diffusion's sub-step count of every row jms..jme in the last call (0 outside its jts..jte)"""
    n = np.zeros(domain.ny, np.int32)
    check(lib().icar_hip_pbl_nsubsteps(domain.ctx, n.ctypes.data_as(ctypes.c_void_p), int(domain.ny)), "icar_hip_pbl_nsubsteps")
    return n


def pbl_finalize(options, domain=None):
    """pbl_driver.f90 pbl_finalize -> finalize_simple_pbl: the context frees its work arrays when it is destroyed; the scheme is
    switched off."""
    if domain is not None:
        check(lib().icar_hip_pbl_configure(domain.ctx, 0), "icar_hip_pbl_configure")
        domain._pbl_key = 0

"""boundary-layer driver mirror (src/physics/pbl_driver.f90): pbl_var_request / pbl_init / pbl / pbl_finalize.

Only the simple scheme (kPBL_SIMPLE, src/physics/pbl_simple.f90, Hong and Pan 1996) is built; kPBL_BASIC has no branch in the
reference's driver either, kPBL_YSU is refused by the library."""
import ctypes
import numpy as np
from .capi import lib, check
from .constants import kPBL_SIMPLE


def pbl_var_request(options):
    """pbl_driver.f90:58-103, as written: the kPBL_SIMPLE block tests options%physics%landsurface (:62), not boundarylayer, so with
    the usual options (land surface off, or any scheme but number 2) choosing the simple PBL requests NOTHING -- the six scalars,
    exner, density, u and v it reads are there because the microphysics and the advection asked for them.  Reproduced, not
    repaired.  (dz_interface, u, v and land_mask are requested for allocation and restart by name; only the first two of the
    list are advected.)"""
    if options.physics.landsurface == kPBL_SIMPLE:
        options.alloc_vars(["water_vapor", "potential_temperature", "cloud_water", "cloud_ice", "rain_in_air", "snow_in_air",
                            "exner", "dz_interface", "density", "u", "v", "land_mask"])
        options.advect_vars(["potential_temperature", "water_vapor"])
        options.restart_vars(["water_vapor", "potential_temperature", "exner", "dz_interface", "density", "u", "v", "land_mask"])


def pbl_init(domain, options):
    """pbl_driver.f90:106-195 -> init_simple_pbl (pbl_simple.f90:296-330 allocates the module's work arrays; here the context
    allocates its own on the first call): hands options%physics%boundarylayer to the library (icar_hip_pbl_configure)."""
    check(lib().icar_hip_pbl_configure(domain.ctx, int(options.physics.boundarylayer)), "icar_hip_pbl_configure")
    domain._pbl_key = int(options.physics.boundarylayer)


def pbl(domain, options, dt):
    """pbl(domain, options, dt_in) (pbl_driver.f90:197-221): simple_pbl on the tile its..kte of the domain's grid, dt a REAL(4)
    like real(dt%seconds()).  The six scalars, u_mass, v_mass, exner, density, z, dz_mass and terrain must be on the device
    (IcarHipError names the missing member); without a land_mask every cell is land."""
    if options.physics.boundarylayer != kPBL_SIMPLE:
        return
    domain.configure(options)
    check(lib().icar_hip_pbl(domain.ctx, float(dt)), "icar_hip_pbl")


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

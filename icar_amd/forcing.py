"""The forcing update of the outer loop (src/main/driver.f90:133-137) on the device: a small mirror of boundary_t and the calls
behind domain_t.interpolate_forcing / .update_delta_fields and this module's forcing_step (include/icar_hip.h, F2).

Arrays are numpy in C order, which is the reference's Fortran order read backwards: a forcing variable (ny_f, nz_f, nx_f), the look-up
tables geolut x / y / w (ny, nx, 4) and vert_lut z / w (ny, nz, nx, 2), indices 1-based as geo_LUT and vLUT leave them."""
import ctypes

import numpy as np

from .capi import lib, check, forcing_geo_c, FORCED2D, FORCED2D_DATA, FORCED2D_DQDT


class geo_t:
    """forcing%geo, %geo_u or %geo_v: the look-up tables onto one of the domain's grids (for u / v the EXTENDED staggered grid, with the
    0-based offset i0, j0 of the tile's staggered grid in it) and, for the mass grid, forcing%geo%z (ny, nz_f, nx)"""

    def __init__(self, x, y, w, z, zw, forcing_shape, i0=0, j0=0, geo_z=None):
        self.x, self.y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
        self.w = np.ascontiguousarray(w, np.float32)
        self.z, self.zw = np.ascontiguousarray(z, np.int32), np.ascontiguousarray(zw, np.float32)
        self.ny_f, self.nz_f, self.nx_f = (int(n) for n in forcing_shape)
        self.i0, self.j0 = int(i0), int(j0)
        self.geo_z = None if geo_z is None else np.ascontiguousarray(geo_z, np.float32)
        ny, nx, four = self.x.shape
        if four != 4 or self.y.shape != self.x.shape or self.w.shape != self.x.shape:
            raise ValueError("geolut x, y, w are (ny, nx, 4)")
        if self.z.ndim != 4 or self.z.shape[0] != ny or self.z.shape[2] != nx or self.z.shape[3] != 2 or self.zw.shape != self.z.shape:
            raise ValueError("vert_lut z, w are (ny, nz, nx, 2) on the grid of the geolut")
        self.ny, self.nx, self.nz = ny, nx, self.z.shape[1]

    def as_c(self):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        return forcing_geo_c(p(self.x), p(self.y), p(self.w), p(self.z), p(self.zw), self.nx, self.ny, self.nx_f, self.nz_f, self.ny_f, self.i0, self.j0)


class boundary_t:
    """variables: {domain member name: the forcing variable's array as just read}; geo, geo_u, geo_v: geo_t (geo_u / geo_v may be None
    when the winds are not forced)"""

    def __init__(self, geo, geo_u=None, geo_v=None, variables=None):
        self.geo, self.geo_u, self.geo_v = geo, geo_u, geo_v
        self.variables = dict(variables or {})


def _ids(domain, names):
    ids = [domain.fid(n) for n in names]
    return (ctypes.c_int * max(len(ids), 1))(*ids), len(ids)


def forcing_configure(domain, forcing, nsmooth=1, domain_z=None, time_varying_z=False):
    """the tables of forcing%geo / %geo_u / %geo_v, domain%nsmooth and, for the pressure adjustment, forcing%geo%z with domain%geo%z"""
    g = forcing.geo
    if g.nz != domain.nz:
        raise ValueError(f"vert_lut has {g.nz} levels, the tile {domain.nz}")
    for s in (forcing.geo_u, forcing.geo_v):
        if s is not None and s.nz != domain.nz:
            raise ValueError(f"vert_lut has {s.nz} levels, the tile {domain.nz}")
    cm = g.as_c()
    cu = forcing.geo_u.as_c() if forcing.geo_u is not None else None
    cv = forcing.geo_v.as_c() if forcing.geo_v is not None else None
    zf = zd = None
    if domain_z is not None:
        zd = np.ascontiguousarray(domain_z, np.float32)
        zf = g.geo_z
        if zf is None or zf.shape != (domain.ny, g.nz_f, domain.nx) or zd.shape != (domain.ny, domain.nz, domain.nx):
            raise ValueError("forcing%geo%z is (ny, nz_f, nx) and domain%geo%z (ny, nz, nx)")
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    ref = lambda c: None if c is None else ctypes.byref(c)
    check(lib().icar_hip_forcing_configure(domain.ctx, ref(cm), ref(cu), ref(cv), int(nsmooth), p(zf), p(zd), int(bool(time_varying_z))),
          "icar_hip_forcing_configure")
    domain._forcing_nsmooth = int(nsmooth)


def forcing_upload(domain, name, array):
    a = np.ascontiguousarray(array, np.float32)
    if a.ndim != 3:
        raise ValueError(f"{name}: a forcing variable is (ny_f, nz_f, nx_f)")
    check(lib().icar_hip_forcing_upload(domain.ctx, domain.fid(name), a.ctypes.data_as(ctypes.c_void_p), a.shape[2], a.shape[1], a.shape[0]),
          f"icar_hip_forcing_upload {name}")


def forcing_download(domain, name, shape):
    a = np.empty(shape, np.float32)
    check(lib().icar_hip_forcing_download(domain.ctx, domain.fid(name), a.ctypes.data_as(ctypes.c_void_p), a.size), f"icar_hip_forcing_download {name}")
    return a


def _special(domain, names, pressure, theta):
    pf = domain.fid(pressure) if pressure in names else -1
    return pf, domain.fid(theta)


def interpolate_forcing(domain, forcing, update=False, pressure="pressure", theta="potential_temperature", upload=True):
    """domain%interpolate_forcing(forcing, update): uploads forcing.variables (upload = False: they are on the device already) and
    interpolates every one of them onto the domain: into dqdt_3d when update, else into the variable itself"""
    names = list(forcing.variables)
    if upload:
        for n in names:
            forcing_upload(domain, n, forcing.variables[n])
    ids, n = _ids(domain, names)
    pf, tf = _special(domain, names, pressure, theta)
    check(lib().icar_hip_interpolate_forcing(domain.ctx, ids, n, pf, tf, int(bool(update))), "icar_hip_interpolate_forcing")
    domain._forced_names = names


def update_delta_fields(domain, dt_seconds, names=None):
    """domain%update_delta_fields(dt) over the variables last interpolated (or `names`) and w"""
    ids, n = _ids(domain, getattr(domain, "_forced_names", []) if names is None else names)
    check(lib().icar_hip_update_delta_fields(domain.ctx, ids, n, ctypes.c_double(dt_seconds)), "icar_hip_update_delta_fields")


def forcing_step(domain, forcing, options, dt_seconds, pressure="pressure", theta="potential_temperature", upload=True, forced_2d=None):
    """driver.f90:133-137 behind boundary%update_forcing: interpolate_forcing(update = .true.), update_winds, update_delta_fields.
    forced_2d = {name: array (ny_f, nx_f)}: these 2-D variables are uploaded and enabled first (forcing2d_enable), so the same call
    interpolates them and takes their delta, and every later sub-step applies them; None leaves the enabled set as it is"""
    if forced_2d is not None:
        for n, a in forced_2d.items():
            forcing2d_upload(domain, n, a)
        forcing2d_enable(domain, list(forced_2d))
    names = list(forcing.variables)
    if upload:
        for n in names:
            forcing_upload(domain, n, forcing.variables[n])
    ids, n = _ids(domain, names)
    pf, tf = _special(domain, names, pressure, theta)
    p = options.parameters
    halo = int(getattr(domain.comm, "halo", 1)) if getattr(domain, "comm", None) is not None else 1      # as icar_amd.wind.update_winds
    check(lib().icar_hip_forcing_step(domain.ctx, ids, n, pf, tf, int(options.physics.windtype), int(p.wind_iterations), ctypes.c_float(domain.dx),
                                      halo, ctypes.c_double(dt_seconds)), "icar_hip_forcing_step")
    domain._forced_names = names


# ---- the 2-D forced variables (include/icar_hip.h, F3): sst, shortwave, longwave, external_precipitation ----------------------------
def _which(names):
    ids = [n if isinstance(n, int) else FORCED2D[n] for n in names]
    return (ctypes.c_int * max(len(ids), 1))(*ids), len(ids)


def _one(name):
    return name if isinstance(name, int) else FORCED2D[name]


def forcing2d_upload(domain, name, array):
    """input_data%data_2d of a 2-D forcing variable, (ny_f, nx_f), as just read"""
    a = np.ascontiguousarray(array, np.float32)
    if a.ndim != 2:
        raise ValueError(f"{name}: a 2-D forcing variable is (ny_f, nx_f)")
    check(lib().icar_hip_forcing2d_upload(domain.ctx, _one(name), a.ctypes.data_as(ctypes.c_void_p), a.shape[1], a.shape[0]), f"icar_hip_forcing2d_upload {name}")


def forcing2d_download(domain, name, shape):
    a = np.empty(shape, np.float32)
    check(lib().icar_hip_forcing2d_download(domain.ctx, _one(name), a.ctypes.data_as(ctypes.c_void_p), a.size), f"icar_hip_forcing2d_download {name}")
    return a


def interpolate_forcing_2d(domain, names, update=False):
    """the two_d branch of domain%interpolate_forcing (domain_obj.f90:2595-2600): geo_interp2d into dqdt_2d when update, else data_2d"""
    ids, n = _which(names)
    check(lib().icar_hip_interpolate_forcing_2d(domain.ctx, ids, n, int(bool(update))), "icar_hip_interpolate_forcing_2d")


def update_delta_fields_2d(domain, names, dt_seconds):
    """domain_obj.f90:2355-2356 for the listed 2-D variables"""
    ids, n = _which(names)
    check(lib().icar_hip_update_delta_fields_2d(domain.ctx, ids, n, ctypes.c_double(dt_seconds)), "icar_hip_update_delta_fields_2d")


def apply_forcing_2d(domain, dt_seconds):
    """domain_obj.f90:2400-2402 and :2438-2445 for the enabled set"""
    check(lib().icar_hip_apply_forcing_2d(domain.ctx, ctypes.c_double(dt_seconds)), "icar_hip_apply_forcing_2d")


def forcing2d_enable(domain, names):
    """the 2-D variables forcing_step and every sub-step handle from now on; an empty list disables"""
    ids, n = _which(names)
    check(lib().icar_hip_forcing2d_enable(domain.ctx, ids, n), "icar_hip_forcing2d_enable")


def forcing2d_get(domain, name, dqdt=False):
    a = np.empty((domain.ny, domain.nx), np.float32)
    check(lib().icar_hip_forcing2d_get(domain.ctx, _one(name), FORCED2D_DQDT if dqdt else FORCED2D_DATA, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_forcing2d_get {name}")
    return a


def forcing2d_set(domain, name, array, dqdt=False):
    a = np.ascontiguousarray(array, np.float32)
    if a.shape != (domain.ny, domain.nx):
        raise ValueError(f"{name}: data_2d and dqdt_2d are (ny, nx)")
    check(lib().icar_hip_forcing2d_set(domain.ctx, _one(name), FORCED2D_DQDT if dqdt else FORCED2D_DATA, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_forcing2d_set {name}")

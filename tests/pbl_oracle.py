"""TEST INFRASTRUCTURE: loader of tests/support/pbl_oracle.c (the CPU restatement of src/physics/pbl_simple.f90) and the recipe of
the boundary-layer test cases.  The library is compiled with gcc -O2 -ffp-contract=off on first use and by
__graft_entry__.build(), so that it exists where the GPU tests run."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "pbl_oracle.c")
LIB = os.path.join(HERE, "support", "libpbl_oracle.so")
SCALARS = ["potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "rain", "snow"]      # simple_pbl's argument order
MEMBER = {"potential_temperature": "potential_temperature", "water_vapor": "water_vapor", "cloud_water": "cloud_water_mass",
          "cloud_ice": "cloud_ice_mass", "rain": "rain_mass", "snow": "snow_mass"}
FLAGS = {"shear_floor": 1, "rig_floor": 2, "rig_pos": 4, "rig_nonpos": 8, "pr_upper": 16, "pr_lower": 32, "kq_upper": 64,
         "kq_lower": 128, "dz_cap": 256, "water": 512, "cell": 1024}
f32 = np.float32
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", LIB, "-lm"])
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def simple_pbl(A, um, vm, exner, density, z, dz, terrain, land_mask, its, ite, jts, jte, kts, kte, dt, flags=False):
    """In place on the six fields of A (SCALARS).  Returns (nsubsteps per row (ny,), flags (ny,nz,nx) or None)."""
    ny, nz, nx = z.shape
    for a in list(A.values()) + [um, vm, exner, density, z, dz, terrain]:
        assert a.dtype == f32 and a.flags.c_contiguous
    assert land_mask is None or (land_mask.dtype == np.int32 and land_mask.flags.c_contiguous)
    nsub = np.zeros(ny, np.int32)
    fl = np.zeros((ny, nz, nx), np.int32) if flags else None
    ci = ctypes.c_int
    rc = lib().pbl_oracle_simple(ci(nx), ci(nz), ci(ny), *[_p(A[k]) for k in SCALARS], _p(um), _p(vm), _p(exner), _p(density), _p(z), _p(dz),
                                 _p(terrain), _p(land_mask), ci(its), ci(ite), ci(jts), ci(jte), ci(kts), ci(kte), ctypes.c_float(dt), _p(nsub), _p(fl))
    if rc:
        raise ValueError("pbl_oracle: no half level between kts and min(nz-1, kte)")
    return nsub, fl


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_pbl.py) and of the GPU tests ----------------------------------
CASES = {"pbl_simple_a_40x36x20": dict(nx=40, ny=36, nz=20, seed=1, rough=6.0, dt=60.0, th_noise=0.5),
         "pbl_simple_b_30x20x40": dict(nx=30, ny=20, nz=40, seed=2, rough=12.0, dt=120.0, th_noise=0.5),
         "pbl_simple_c_calm_24x12x12": dict(nx=24, ny=12, nz=12, seed=3, rough=0.0, dt=30.0, th_noise=0.5),
         "pbl_simple_d_26x14x3": dict(nx=26, ny=14, nz=3, seed=4, rough=8.0, dt=90.0, th_noise=0.5),
         "pbl_simple_e_20x12x24": dict(nx=20, ny=12, nz=24, seed=5, rough=40.0, dt=120.0, th_noise=2.0)}
CALLS = 3


def mass_heights(c):
    """domain%z%data_3d of an ideal case: terrain + level centre x jacobian"""
    dzl = c["dz_levels"].astype(np.float64)
    zi = np.concatenate([[0.0], np.cumsum(dzl)]); zc = 0.5 * (zi[1:] + zi[:-1])
    jac = c["jacobian"][:, 0, :].astype(np.float64)
    return (c["terrain"][:, None, :] + zc[None, :, None] * jac[:, None, :]).astype(f32), zc


def make_case(nx, ny, nz, seed, rough, dt, th_noise=0.5, hill=800.0, water=0.2, uniform_dz=None, dx=1000.0):
    """Fields of icar_amd.ideal plus sheared mass-point winds with row-wise patchy noise (row amplitude = rough x random**3: calm
    and rough rows alternate, so that the rows' sub-step counts differ), +-th_noise K of noise on theta (stable and unstable
    layers) and `water` of the cells water.  Returns a dict: the ideal case's members, z, u_mass, v_mass, land_mask, dt."""
    from icar_amd import ideal
    c = ideal.make_case(nx, ny, nz, hill_height=hill, noise=0.03, seed=seed, n_hydro=1, uniform_dz=uniform_dz, dx=dx)
    rng = np.random.default_rng(seed)
    z, zc = mass_heights(c)
    sh = (ny, nz, nx)
    amp = rough * (rng.random((ny, 1, 1)) ** 3)
    c["u_mass"] = (10.0 + 3 * np.log1p(zc / 50.0)[None, :, None] + amp * rng.standard_normal(sh)).astype(f32)
    c["v_mass"] = (3.0 + amp * rng.standard_normal(sh)).astype(f32)
    c["land_mask"] = np.where(rng.random((ny, nx)) < water, 2, 1).astype(np.int32)
    c["potential_temperature"] = (c["potential_temperature"] + (th_noise * rng.standard_normal(sh)).astype(f32)).astype(f32)
    c["z"] = z
    c["pbl_dt"] = float(dt)
    return c


def state(c):
    return {k: np.ascontiguousarray(c[k], f32).copy() for k in SCALARS}


def run_oracle(c, A, tile=None, kts=1, kte=None, flags=False, land=True):
    ny, nz, nx = c["z"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    return simple_pbl(A, c["u_mass"], c["v_mass"], c["exner"], c["density"], c["z"], c["dz_mass"], c["terrain"],
                      c["land_mask"] if land else None, its, ite, jts, jte, kts, nz if kte is None else kte, c["pbl_dt"], flags=flags)


def device_domain(c, land=True):
    """a single-image domain_t holding the case (terrain, z, u_mass, v_mass and, unless land=False, land_mask included)"""
    from util import single_image_domain
    if not land:
        c = {k: v for k, v in c.items() if k != "land_mask"}
    return single_image_domain(c)


def device_state(d):
    return {k: d.get(MEMBER[k]) for k in SCALARS}


def bitdiff(a, b):
    return int((np.ascontiguousarray(a).view(np.int32) != np.ascontiguousarray(b).view(np.int32)).sum())


def fingerprint(c):
    return float(sum(float(np.asarray(c[k], np.float64).sum()) for k in SCALARS + ["u_mass", "v_mass", "exner", "density", "z", "dz_mass", "terrain", "land_mask"]))

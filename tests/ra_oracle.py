"""TEST INFRASTRUCTURE: loader of tests/support/ra_oracle.c (the CPU restatement of src/physics/ra_simple.f90) and the recipe of
the radiation test cases.  The library is compiled with gcc -O2 -ffp-contract=off on first use and by
__graft_entry__.build(), so that it exists where the GPU tests run."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "ra_oracle.c")
LIB = os.path.join(HERE, "support", "libra_oracle.so")
INPUTS = ["potential_temperature", "exner", "water_vapor", "cloud_water", "snow", "cloud_ice", "graupel", "rain", "pressure"]   # ra_simple's argument order (qs = snow + ice + graupel)
OUTPUTS = ["potential_temperature", "shortwave", "longwave", "cloud_fraction"]
FLAGS = {"night": 1, "asin_clip": 2, "lon_gt_180": 4, "rh_at_1": 8, "hydro_clip": 16, "qc_floor": 32, "temp_floor": 64, "cf_at_1": 128,
         "lw_cap": 256, "cell": 512}
GREGORIAN, NOLEAP, THREESIXTY = 0, 1, 2
SENTINEL = -7.0                 # what shortwave / longwave / cloud_fraction hold before the first call
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


def ra_simple(A, c, D, year_days, calendar, dt, its, ite, jts, jte, kts, kte, runlw=True, flags=False):
    """In place on A["potential_temperature"], A["shortwave"], A["longwave"], A["cloud_fraction"]; the other inputs from c.
    Returns the flags (ny, nx) or None."""
    ny, nz, nx = A["potential_temperature"].shape
    arr = [A["potential_temperature"]] + [c[k] for k in INPUTS[1:]] + [A["shortwave"], A["longwave"], A["cloud_fraction"], c["latitude"], c["longitude"]]
    for a in arr:
        assert a.dtype == f32 and a.flags.c_contiguous
    fl = np.zeros((ny, nx), np.int32) if flags else None
    ci = ctypes.c_int
    rc = lib().ra_oracle_simple(ci(nx), ci(nz), ci(ny), *[_p(a) for a in arr], ctypes.c_double(D), ctypes.c_double(year_days), ci(calendar),
                                ctypes.c_float(dt), ci(its), ci(ite), ci(jts), ci(jte), ci(kts), ci(kte), ci(int(runlw)), _p(fl))
    if rc:
        raise ValueError("ra_oracle: ra_simple: at least 5 levels")
    return fl


def libm(which, x):
    """sinf / cosf / asinf of the host's C library on a REAL(4) array"""
    x = np.ascontiguousarray(x, f32)
    y = np.empty_like(x)
    lib().ra_oracle_libm(ctypes.c_int({"sinf": 0, "cosf": 1, "asinf": 2}[which]), ctypes.c_long(x.size), _p(x), _p(y))
    return y


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_ra.py) and of the GPU tests ----------------------------------
# D0: days since 1 January 00:00 at the first call; advance: seconds of model time between calls; dt: the first call's dt (the
# n-th call takes dt x n); year_days / next_year_days: the calendar anchor; subsolar: share of the columns put at the point where
# the sun stands in the zenith at the first call (the only place where rounding takes sin(elevation) past 1)
CASES = {"ra_simple_a_40x36x20": dict(nx=40, ny=36, nz=20, seed=1, calendar=GREGORIAN, D0=60.25, year_days=366, next_year_days=365, advance=21600.0, dt=60.0),
         "ra_simple_b_noleap_26x14x5": dict(nx=26, ny=14, nz=5, seed=2, calendar=NOLEAP, D0=172.70, year_days=365, next_year_days=365, advance=3600.0, dt=120.0),
         "ra_simple_c_360day_66x12x24": dict(nx=66, ny=12, nz=24, seed=3, calendar=THREESIXTY, D0=265.20, year_days=360, next_year_days=360, advance=1800.0, dt=30.0),
         "ra_simple_d_norunlw_30x20x12": dict(nx=30, ny=20, nz=12, seed=4, calendar=GREGORIAN, D0=200.5, year_days=365, next_year_days=365, advance=43200.0, dt=90.0, runlw=False),
         "ra_simple_e_newyear_24x12x8": dict(nx=24, ny=12, nz=8, seed=5, calendar=GREGORIAN, D0=364.85, year_days=365, next_year_days=366, advance=10800.0, dt=100.0),
         "ra_simple_f_zenith_40x20x6": dict(nx=40, ny=20, nz=6, seed=6, calendar=GREGORIAN, D0=25.5, year_days=365, next_year_days=365, advance=600.0, dt=20.0, subsolar=0.8)}
CALLS = 3


def make_case(nx, ny, nz, seed, calendar=GREGORIAN, D0=60.25, year_days=365, next_year_days=365, advance=3600.0, dt=60.0, runlw=True,
              subsolar=0.0, hill=500.0, dx=4000.0, uniform_dz=None):
    """Fields of icar_amd.ideal plus what the scheme's branches need: latitudes -90 .. 90 along j (the poles exactly) and
    longitudes -180 .. 360 along i, both with noise; columns saturated over the lowest five levels (the mean rh at its cap 1),
    warm columns (+30 K: the 600 W/m2 cap), and per column one of four hydrometeor classes -- none, traces below qcmin (the 5e-8
    floor), clouds, and negative leftovers (the clip at 0) -- of all five species, signs mixed inside a column.  uniform_dz: levels
    of that thickness instead of the stretched ones (tall columns: the ideal profiles are defined below ~44 km)."""
    from icar_amd import ideal
    c = ideal.make_case(nx, ny, nz, hill_height=hill, noise=0.03, seed=seed, dx=dx, uniform_dz=uniform_dz)
    rng = np.random.default_rng(seed)
    sh = (ny, nz, nx)
    lat = np.linspace(-90.0, 90.0, ny)[:, None] + np.where((np.arange(ny) % (ny - 1) == 0)[:, None], 0.0, rng.uniform(-2, 2, (ny, nx)))
    lon = np.linspace(-180.0, 360.0, nx)[None, :] + rng.uniform(-3, 3, (ny, nx))
    lon = np.clip(lon, -180.0, 360.0)
    if subsolar > 0:
        # local noon (hour angle 0) where D0 + lon / 360 ends in .5; the declination of that day as a latitude
        doy = D0 + 0.0
        lon0 = ((0.5 - (D0 % 1.0)) * 360.0 + 180.0) % 360.0 - 180.0
        decl = -0.4091 * np.cos(2.0 * np.pi / 365.0 * (doy + lon0 / 360.0 + 10.0))
        at = rng.random((ny, nx)) < subsolar
        lat = np.where(at, np.degrees(decl) + rng.uniform(-0.004, 0.004, (ny, nx)), lat)
        lon = np.where(at, lon0 + rng.uniform(-0.004, 0.004, (ny, nx)), lon)
    c["latitude"] = np.clip(lat, -90.0, 90.0).astype(f32)
    c["longitude"] = lon.astype(f32)
    warm = rng.random((ny, 1, nx)) < 0.12
    c["potential_temperature"] = (c["potential_temperature"] + np.where(warm, 30.0, 0.0) + 0.5 * rng.standard_normal(sh)).astype(f32)
    T = c["potential_temperature"].astype(np.float64) * c["exner"]
    wet = rng.random((ny, 1, nx)) < 0.25
    c["water_vapor"] = np.where(wet, 1.3 * ideal.sat_mr(T, c["pressure"]), c["water_vapor"] * rng.uniform(0.3, 1.1, sh)).astype(f32)
    cls = rng.integers(0, 4, (ny, 1, nx))
    amp = np.select([cls == 0, cls == 1, cls == 2, cls == 3], [0.0, 2e-9, 10.0 ** rng.uniform(-7.0, -4.0, (ny, 1, nx)), -3e-7])
    for n, k in enumerate(("cloud_water", "rain", "snow", "cloud_ice", "graupel")):
        c[k] = (amp * rng.uniform(-0.3, 1.0, sh)).astype(f32)
    c.update(calendar=int(calendar), D0=float(D0), year_days=int(year_days), next_year_days=int(next_year_days), advance=float(advance),
             ra_dt=float(dt), runlw=bool(runlw))
    return c


def seconds(c, n):
    """the model clock at call n (0-based), in seconds since 1 January 00:00 of the first call's year"""
    return float(round(c["D0"] * 86400.0)) + n * c["advance"]


def clock(c, n):
    """(D, year_days) of call n (0-based): the day of the year as the library forms it from the clock -- seconds / 86400 in FP64,
    rolled once into the next year"""
    D = seconds(c, n) / 86400.0
    if D >= c["year_days"]:
        return D - c["year_days"], c["next_year_days"]
    return D, c["year_days"]


def state(c):
    ny, nz, nx = c["pressure"].shape
    A = {"potential_temperature": np.ascontiguousarray(c["potential_temperature"], f32).copy()}
    for k in OUTPUTS[1:]:
        A[k] = np.full((ny, nx), SENTINEL, f32)
    return A


def run_oracle(c, A, n=0, tile=None, kts=1, kte=None, flags=False, runlw=None):
    """call n (0-based) of the carried sequence: dt x (n + 1) at the clock of clock(c, n)"""
    ny, nz, nx = c["pressure"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    D, yd = clock(c, n)
    return ra_simple(A, c, D, yd, c["calendar"], c["ra_dt"] * (n + 1), its, ite, jts, jte, kts, nz if kte is None else kte,
                     runlw=c["runlw"] if runlw is None else runlw, flags=flags)


def device_domain(c):
    """a single-image domain_t holding the case (latitude and longitude included), the three results at SENTINEL, the calendar
    anchored so that the library clock counts seconds since 1 January 00:00 of the first call's year"""
    from util import single_image_domain
    from icar_amd import radiation
    d = single_image_domain(c)
    for k in OUTPUTS[1:]:
        d.set(k, np.full((d.ny, d.nx), SENTINEL, f32))
    radiation.rad_calendar(d, c["calendar"], 0.0, c["year_days"], c["next_year_days"])
    return d


def device_call(d, c, n=0, tile=None, kts=1, kte=None, runlw=None):
    """call n of the carried sequence on the device: the clock of seconds(c, n), dt x (n + 1)"""
    from icar_amd import radiation
    ny, nz, nx = c["pressure"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    d.model_time_seconds = seconds(c, n)
    radiation.ra_simple(d, c["ra_dt"] * (n + 1), its, ite, jts, jte, kts, nz if kte is None else kte, runlw=c["runlw"] if runlw is None else runlw)


def device_state(d):
    return {k: d.get(k) for k in OUTPUTS}


def bitdiff(a, b):
    return int((np.ascontiguousarray(a).view(np.int32) != np.ascontiguousarray(b).view(np.int32)).sum())


def tile_mask(c, tile=None):
    ny, nz, nx = c["pressure"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    m = np.zeros((ny, nx), bool); m[jts - 1:jte, its - 1:ite] = True
    rows = np.zeros((ny, nx), bool); rows[jts - 1:jte, :] = True
    return m, rows


def fingerprint(c):
    return float(sum(float(np.asarray(c[k], np.float64).sum()) for k in INPUTS + ["latitude", "longitude"]))

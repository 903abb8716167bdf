"""TEST INFRASTRUCTURE: loader of tests/support/bmj_oracle.c (the CPU restatement of the convection slot with convection = kCU_BMJ: the
product's own column header icar_amd/csrc/bmj_column.h compiled for the host, BMJINIT's tables, convect's streaming statements) and
the recipe of the convection test cases.  The library is compiled with gcc -O2 -ffp-contract=off on first use and by
__graft_entry__.build(), so that it exists where the GPU tests run."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "bmj_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "bmj_column.h")
LIB = os.path.join(HERE, "support", "libbmj_oracle.so")
f32 = np.float32
kCU_BMJ = 5
NONE, DEEP, SHALLOW = 0, 1, 2
TABLES = [("QS0", (134,)), ("SQS", (134,)), ("PTBL", (134, 76)), ("THE0", (76,)), ("STHE", (76,)), ("TTBL", (76, 134)),
          ("THE0Q", (152,)), ("STHEQ", (152,)), ("TTBLQ", (152, 440))]          # C shapes of the Fortran arrays (last index first)
STATE3 = ["potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "tend_th", "tend_qv"]
STATE2 = ["cldefi", "raincv", "cutop", "cubot", "accumulated_convective_pcp"]
INPUT3 = ["pressure", "pressure_interface", "exner", "density", "dz_interface"]
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(LIB):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", LIB, "-lm"])
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.bmj_oracle_avgefi.restype = ctypes.c_float
        _lib.bmj_oracle_efimn.restype = ctypes.c_float
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def tables():
    """{name: array} of BMJINIT's nine tables as the restatement builds them"""
    n = lib().bmj_oracle_table_floats()
    block = np.zeros(n, f32)
    lib().bmj_oracle_tables(_p(block))
    out, o = {}, 0
    for name, shape in TABLES:
        cnt = int(np.prod(shape))
        out[name] = block[o:o + cnt].reshape(shape).copy()
        o += cnt
    assert o == n
    return out


AVGEFI = lambda: float(lib().bmj_oracle_avgefi())
EFIMN = lambda: float(lib().bmj_oracle_efimn())
MAX_LEVELS = lambda: int(lib().bmj_oracle_max_levels())          # of the scheme: kte - kts
MIN_NZ = 3                                                       # kte - kts + 1 >= 3: with one scheme level the reference reads PRSMID(LBOT+1) past the column


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_bmj.py) and of the GPU tests --------------------------------
# dt: the three carried calls' time steps; fractions: tendency_fraction and the four fractions (negative: inherit, options_obj.f90:1646)
CASES = {"cu_bmj_a_32x24x12": dict(nx=32, ny=24, nz=12, seed=1),
         "cu_bmj_b_8lev_26x14x8": dict(nx=26, ny=14, nz=8, seed=2),
         "cu_bmj_c_64lev_20x12x64": dict(nx=20, ny=12, nz=64, seed=3, rh_lo=0.6),
         "cu_bmj_d_thzero_30x20x20": dict(nx=30, ny=20, nz=20, seed=4, tend_th_fraction=0.0),
         "cu_bmj_e_half_20x10x90": dict(nx=20, ny=10, nz=90, seed=5, tendency_fraction=0.5, rh_lo=0.85),
         "cu_bmj_f_negzero_34x10x41": dict(nx=34, ny=10, nz=41, seed=6, negzero=True, cldefi0=0.95, rh_lo=0.8)}
CALLS = 3
DT = (20.0, 40.0, 60.0)


def sounding(nx, ny, nz, seed, noise=True, rh_lo=0.25):
    """The probe sounding of the convection slot: surface temperature 284..306 K along i, 6.5 K/km down to a 210 K floor, relative
    humidity rh_lo = 0.25..0.97 along j held below 1.5 km and decaying above it with a 3..7 km scale (along i), a 16 km lid with the layer
    thickness proportional to 0.5 + k/nz, surface pressure 978..1000 hPa, land and sea alternating (with a few 0 = water of a
    LANDMASK input).  Hydrostatic, in FP64, rounded once to REAL(4); the diagnostics are those diagnostic_update would leave."""
    rng = np.random.default_rng(4000 + seed)
    s3, s2 = (ny, nz, nx), (ny, nx)
    w = 0.5 + np.arange(nz) / nz
    dzl = 16000.0 * w / w.sum()
    dz = np.broadcast_to(dzl[None, :, None], s3) * (rng.uniform(0.985, 1.0, s3) if noise else 1.0)
    zi = np.concatenate([np.zeros((ny, 1, nx)), np.cumsum(dz, axis=1)], axis=1)          # interfaces, nz+1
    z = 0.5 * (zi[:, :-1] + zi[:, 1:])
    fi = (np.arange(nx) / max(nx - 1, 1))[None, :]
    fj = (np.arange(ny) / max(ny - 1, 1))[:, None]
    tsfc = 284.0 + 22.0 * fi + np.zeros(s2)
    psfc = 97800.0 + 2200.0 * rng.random(s2)
    # a warm layer aloft over every third column (3..9 K around zinv = 2.2..3.4 km): the cap under which the cloud stays shallow
    cap = np.where((np.arange(nx)[None, :] + 2 * np.arange(ny)[:, None]) % 3 == 0, 3.0 + 6.0 * rng.random(s2), 0.0)
    zinv = 2200.0 + 1200.0 * rng.random(s2)
    T = np.maximum(210.0, tsfc[:, None, :] - 0.0065 * z) + cap[:, None, :] * np.exp(-((z - zinv[:, None, :]) / 900.0) ** 2)
    T = T + (rng.normal(0, 0.05, s3) if noise else 0.0)
    Rd, g, cp = 287.058, 9.81, 1012.0
    pint = np.empty((ny, nz + 1, nx)); pint[:, 0] = psfc
    for k in range(nz):
        pint[:, k + 1] = pint[:, k] * np.exp(-g * dz[:, k] / (Rd * T[:, k]))
    p = np.sqrt(pint[:, :-1] * pint[:, 1:])
    rh0 = rh_lo + (0.97 - rh_lo) * fj + np.zeros(s2)
    H = 3000.0 + 4000.0 * fi + np.zeros(s2)
    rh = rh0[:, None, :] * np.where(z < 1500.0, 1.0, np.exp(-(z - 1500.0) / H[:, None, :]))
    es = 610.78 * np.exp(17.2693882 * (T - 273.16) / (T - 35.86))
    qs = 0.622 * es / np.maximum(p - es, 1.0)
    qv = np.maximum(rh * qs, 1e-7)
    lm = np.where((np.arange(nx)[None, :] + np.arange(ny)[:, None]) % 2 == 0, 1, 2)
    lm = np.where(rng.random(s2) < 0.05, 0, lm).astype(np.int32)
    p4, T4 = p.astype(f32), T.astype(f32)
    exner = ((p4.astype(np.float64) / 1e5) ** (Rd / cp)).astype(f32)
    return dict(nx=nx, ny=ny, nz=nz, dx=f32(2000.0), dz_interface=dz.astype(f32), z=z.astype(f32), pressure=p4,
                pressure_interface=np.ascontiguousarray(pint[:, :nz]).astype(f32), temperature=T4, exner=exner,
                potential_temperature=(T4 / exner).astype(f32), density=(p4 / (f32(Rd) * T4)).astype(f32), water_vapor=qv.astype(f32),
                land_mask=lm)


def make_case(nx, ny, nz, seed, tendency_fraction=1.0, tend_qv_fraction=-1.0, tend_qc_fraction=-1.0, tend_th_fraction=-1.0,
              tend_qi_fraction=-1.0, negzero=False, cldefi0=0.6, noise=True, rh_lo=0.25):
    c = sounding(nx, ny, nz, seed, noise, rh_lo)
    rng = np.random.default_rng(5000 + seed)
    s3 = (ny, nz, nx)
    qc = np.where(rng.random(s3) < 0.2, rng.uniform(0, 3e-4, s3), 0.0).astype(f32)
    qi = np.where(rng.random(s3) < 0.1, rng.uniform(0, 1e-4, s3), 0.0).astype(f32)
    if negzero:
        qc[ny // 2, 1, nx // 2] = f32(-0.0)                                # inside the tile
        qi[1, 2, 0] = f32(-0.0)                                            # owned row, halo column
    fr = [tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction]
    fr = [tendency_fraction if f < 0 else f for f in fr]                   # options_obj.f90:1646-1649
    c.update(cloud_water=qc, cloud_ice=qi, cldefi0=float(cldefi0), tendency_fraction=float(tendency_fraction), fractions=[float(f) for f in fr],
             negzero=bool(negzero))
    return c


def state(c):
    """what the slot carries from call to call"""
    ny, nz, nx = c["density"].shape
    A = {k: np.ascontiguousarray(c[k], f32).copy() for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature")}
    A["tend_th"] = np.zeros((ny, nz, nx), f32); A["tend_qv"] = np.zeros((ny, nz, nx), f32)
    A["cldefi"] = np.full((ny, nx), c["cldefi0"], f32)
    for k in ("raincv", "cutop", "cubot", "accumulated_convective_pcp"):
        A[k] = np.zeros((ny, nx), f32)
    A["accumulated_precipitation"] = np.zeros((ny, nx), np.float64)
    return A


def tile_of(c):
    ny, nz, nx = c["density"].shape
    return (2, nx - 1, 2, ny - 1) if nx > 3 and ny > 3 else (1, nx, 1, ny)


def drv(c, A, dt, tile=None, kte=None):
    """BMJDRV alone on the tile; returns the kind of every column (ny, nx)"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or tile_of(c)
    kind = np.zeros((ny, nx), np.int32)
    ci = ctypes.c_int
    rc = lib().bmj_oracle_drv(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ci(nz if kte is None else kte), ctypes.c_float(dt),
                              _p(A["temperature"]), _p(A["water_vapor"]), _p(c["pressure"]), _p(c["pressure_interface"]), _p(c["exner"]),
                              _p(c["density"]), _p(c["dz_interface"]), _p(c["land_mask"]), _p(A["cldefi"]), _p(A["raincv"]), _p(A["cutop"]),
                              _p(A["cubot"]), _p(A["tend_th"]), _p(A["tend_qv"]), _p(kind))
    if rc:
        raise ValueError("bmj_oracle: level count refused")
    return kind


def convect(c, A, dt, tile=None, kte=None):
    """convect(domain, options, dt) on the tile; returns the kind of every column"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or tile_of(c)
    kind = np.zeros((ny, nx), np.int32)
    ci, cf = ctypes.c_int, ctypes.c_float
    fq = c["fractions"]
    rc = lib().bmj_oracle_convect(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ci(nz if kte is None else kte), cf(dt),
                                  _p(A["temperature"]), _p(A["water_vapor"]), _p(A["potential_temperature"]), _p(A["cloud_water"]),
                                  _p(A["cloud_ice"]), _p(c["pressure"]), _p(c["pressure_interface"]), _p(c["exner"]), _p(c["density"]),
                                  _p(c["dz_interface"]), _p(c["land_mask"]), _p(A["cldefi"]), _p(A["raincv"]), _p(A["cutop"]), _p(A["cubot"]),
                                  _p(A["tend_th"]), _p(A["tend_qv"]), _p(A["accumulated_precipitation"]), _p(A["accumulated_convective_pcp"]),
                                  cf(c["tendency_fraction"]), cf(fq[0]), cf(fq[1]), cf(fq[2]), cf(fq[3]), _p(kind))
    if rc:
        raise ValueError("bmj_oracle: level count refused")
    return kind


def rediagnose(c, A):
    """what diagnostic_update does to domain%temperature in front of the next call (time_step.f90: T = theta exner)"""
    A["temperature"] = (A["potential_temperature"] * c["exner"]).astype(f32)


def run_oracle(c, A, n, tile=None):
    """call n (0-based) of the carried sequence: diagnostic_update's temperature (from the second call on), then convect with DT[n]"""
    if n:
        rediagnose(c, A)
    return convect(c, A, DT[n], tile)


def bitdiff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    v = np.int64 if a.dtype == np.float64 else np.int32
    return int((a.view(v) != b.view(v)).sum())


def fingerprint(c):
    return float(sum(float(np.asarray(c[k], np.float64).sum()) for k in INPUT3 + ["temperature", "potential_temperature", "water_vapor",
                                                                                   "cloud_water", "cloud_ice", "land_mask"]))


def owned(c, a, tile=None):
    its, ite, jts, jte = tile or tile_of(c)
    return a[jts - 1:jte, ..., its - 1:ite]


def kinds_share(c, kind, tile=None):
    k = owned(c, kind, tile)
    return {"deep": float((k == DEEP).mean()), "shallow": float((k == SHALLOW).mean()), "none": float((k == NONE).mean())}


# ---- the same on the device -------------------------------------------------------------------------------------------------------
DEVICE_NAME = {"cloud_water": "cloud_water_mass", "cloud_ice": "cloud_ice_mass"}
CU_ARRAYS = ["cldefi", "raincv", "cutop", "cubot", "accumulated_convective_pcp", "tend_th", "tend_qv"]


def options_of(c):
    from icar_amd.options import options_t
    opt = options_t()
    opt.physics.convection = kCU_BMJ
    opt.physics.advection = opt.physics.microphysics = 0
    o = opt.cu_options
    o.tendency_fraction = c["tendency_fraction"]
    o.tend_qv_fraction, o.tend_qc_fraction, o.tend_th_fraction, o.tend_qi_fraction = c["fractions"]
    return opt


def device_domain(c, grid=None):
    """a single-image domain_t holding the case, the slot configured with the case's options and CLDEFI at the case's start value"""
    from util import single_image_domain
    from icar_amd import convection
    from icar_amd.domain import domain_t
    if grid is None:
        d = single_image_domain(c)
    else:
        d = domain_t(grid, device=0, dx=float(c["dx"]))
        d.load_case(c)
    d._cu_opt = options_of(c)
    convection.init_convection(d, d._cu_opt)
    convection.cu_set(d, "cldefi", np.full((d.ny, d.nx), c["cldefi0"], f32))
    d.fill("accumulated_precipitation", 0.0)                           # the host's domain%accumulated_precipitation: the scheme alone never makes it
    return d


def device_call(d, c, n, dt=None):
    """call n of the carried sequence on the device: domain%temperature made again as diagnostic_update makes it (from the second
    call on), then icar_hip_convect on the tile of the domain's grid"""
    from icar_amd import convection
    if n:
        d.set("temperature", (d.get("potential_temperature") * c["exner"]).astype(f32))
    convection.convect(d, d._cu_opt, DT[n] if dt is None else dt)


def device_state(d):
    from icar_amd import convection
    out = {k: d.get(DEVICE_NAME.get(k, k)) for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "accumulated_precipitation")}
    out.update({k: convection.cu_get(d, k) for k in CU_ARRAYS})
    return out

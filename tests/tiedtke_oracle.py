"""TEST INFRASTRUCTURE: loader of tests/support/tiedtke_oracle.c (the CPU restatement of CU_TIEDTKE as cu_driver.f90 calls it: the
product's own column header icar_amd/csrc/tiedtke_column.h compiled for the host) and the recipe of the Tiedtke test cases.  The
library is compiled with gcc -O2 -ffp-contract=off on first use and by __graft_entry__.build()."""
import ctypes
import os
import subprocess

import numpy as np

import bmj_oracle as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "tiedtke_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "tiedtke_column.h")
LIB = os.path.join(HERE, "support", "libtiedtke_oracle.so")
f32 = np.float32
kCU_TIEDTKE = 1
# tdk_column's flags (icar_amd/csrc/tiedtke_column.h)
D_MIDLEVEL, D_CLOUD, D_DOWNDRAFT, D_MELT, D_EVAP, D_ICE, D_WATER = 1, 2, 4, 8, 16, 32, 64
D_PCTE_WARM, D_PCTE_COLD, D_PCTE_MIXED, D_PRECIP, D_SECOND_LOST, D_MFMAX = 128, 256, 512, 1024, 2048, 4096
TEND = ["tend_th", "tend_qv", "tend_qc", "tend_qi"]
OUT2 = ["raincv", "pratec"]
INPUT3 = ["pressure", "pressure_interface", "exner", "density", "dz_interface", "w_real"]
_lib = None
bitdiff = B.bitdiff
owned = B.owned
tile_of = B.tile_of


def build(force=False):
    if force or not os.path.exists(LIB) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(LIB):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", LIB, "-lm"])
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


_p = B._p
MIN_LEVELS = lambda: int(lib().tiedtke_oracle_min_levels())      # of the scheme: kte - 1
MAX_LEVELS = lambda: int(lib().tiedtke_oracle_max_levels())
MIN_NZ = 4                                                       # kte - 1 >= 3: with two scheme levels the reference reads PAPH(JL,0) (cu_tiedtke.f90:937)


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_tiedtke.py) and of the GPU tests ---------------------------
CASES = {"cu_tiedtke_a_terrain_28x18x40": dict(nx=28, ny=18, nz=40, seed=1, terrain=True, lid=9000.0, base_max=7000.0),
         "cu_tiedtke_b_4lev_26x14x4": dict(nx=26, ny=14, nz=4, seed=2),
         "cu_tiedtke_c_64lev_cold_20x12x64": dict(nx=20, ny=12, nz=64, seed=3, t_offset=-14.0, depth_max=9500.0),
         "cu_tiedtke_d_90lev_20x10x90": dict(nx=20, ny=10, nz=90, seed=4, terrain=True, lid=12000.0, wmax=4.0),
         "cu_tiedtke_e_negzero_30x12x30": dict(nx=30, ny=12, nz=30, seed=5, negzero=True),
         "cu_tiedtke_f_water_24x12x40": dict(nx=24, ny=12, nz=40, seed=6, water=True)}
SEEDS = {"seed_g": dict(nx=22, ny=10, nz=36, seed=7, terrain=True), "seed_h": dict(nx=18, ny=9, nz=21, seed=8)}
CALLS = 2
DT = (60.0, 120.0)


def make_case(nx, ny, nz, seed, terrain=False, negzero=False, water=False, lid=16000.0, t_offset=0.0, depth_max=5000.0, wmax=1.5, base_max=4000.0):
    """bmj_oracle's sounding (hydrostatic, FP64 rounded once) with what the Tiedtke scheme reads beside it: a saturated layer aloft
    over part of the columns (the air from which mid-level convection starts, 1.5 .. 5 km deep from 1.5 .. 4 km up), w_real with
    ascent there and weak subsidence elsewhere, znu, and -- terrain -- a surface pressure that falls by up to 300 hPa along i and j,
    so that the interface that stands within 50 hPa of 250 hPa is another one from column to column and from row to row (with a
    lid of 9 km some columns have none: their rows' leveltop is the cap KLEV-15, and which column is first decides who convects).
    t_offset cools the whole sounding (cloud tops below 233 K), depth_max deepens the moist layer, wmax is the strongest ascent, base_max the highest base of the moist layer (near the 250 hPa
    level it makes leveltop decide whether a column convects)."""
    rng = np.random.default_rng(7000 + seed)
    c = B.sounding(nx, ny, nz, seed, True, 0.35)
    s3, s2 = (ny, nz, nx), (ny, nx)
    if t_offset:
        c["temperature"] = (c["temperature"].astype(np.float64) + t_offset).astype(f32)
    if lid != 16000.0 or terrain or t_offset:
        # redo the hydrostatic integration from another surface pressure (and lid) with the sounding's own temperatures
        Rd, g, cp = 287.058, 9.81, 1012.0
        dz = c["dz_interface"].astype(np.float64) * (lid / 16000.0)
        fi = (np.arange(nx) / max(nx - 1, 1))[None, :]
        fj = (np.arange(ny) / max(ny - 1, 1))[:, None]
        if lid != 16000.0:                                                   # the sounding's lapse rate at the new heights
            zn = np.cumsum(dz, axis=1) - 0.5 * dz
            c["temperature"] = (np.maximum(210.0, (284.0 + t_offset + 22.0 * fi)[:, None, :] - 0.0065 * zn) + rng.normal(0, 0.05, s3)).astype(f32)
        T = c["temperature"].astype(np.float64)
        psfc = c["pressure_interface"][:, 0].astype(np.float64) - (30000.0 * (0.6 * fi + 0.4 * fj) if terrain else 0.0)
        pint = np.empty((ny, nz + 1, nx)); pint[:, 0] = psfc
        for k in range(nz):
            pint[:, k + 1] = pint[:, k] * np.exp(-g * dz[:, k] / (Rd * T[:, k]))
        p = np.sqrt(pint[:, :-1] * pint[:, 1:])
        zi = np.concatenate([np.zeros((ny, 1, nx)), np.cumsum(dz, axis=1)], axis=1)
        p4 = p.astype(f32)
        exner = ((p4.astype(np.float64) / 1e5) ** (Rd / cp)).astype(f32)
        T4 = c["temperature"]
        c.update(dz_interface=dz.astype(f32), z=(0.5 * (zi[:, :-1] + zi[:, 1:])).astype(f32), pressure=p4,
                 pressure_interface=np.ascontiguousarray(pint[:, :nz]).astype(f32), exner=exner,
                 potential_temperature=(T4 / exner).astype(f32), density=(p4 / (f32(Rd) * T4)).astype(f32))
    z = c["z"].astype(np.float64)
    T, p = c["temperature"].astype(np.float64), c["pressure"].astype(np.float64)
    es = 610.78 * np.exp(np.where(T > 273.16, 17.269 * (T - 273.16) / (T - 35.86), 21.875 * (T - 273.16) / (T - 7.66)))
    qs = 0.622 * es / np.maximum(p - 0.378 * es, 1.0)
    moist = rng.random(s2) < 0.55                                            # the other columns stay as dry aloft as the sounding is
    base = 1500.0 + (base_max - 1500.0) * rng.random(s2)
    depth = 1500.0 + (depth_max - 1500.0) * rng.random(s2)
    rhm = 0.78 + 0.22 * rng.random(s2)                                       # some layers stay under the 80 % that CUBASMC asks for
    layer = moist[:, None, :] & (z > base[:, None, :]) & (z < (base + depth)[:, None, :])
    qv = np.where(layer, np.maximum(rhm[:, None, :] * qs / (1.0 - rhm[:, None, :] * qs), c["water_vapor"]), c["water_vapor"])
    wamp = np.where(moist, rng.uniform(-0.05, wmax, s2), rng.uniform(-0.05, 0.02, s2))
    zw = np.concatenate([np.zeros((ny, 1, nx)), np.cumsum(c["dz_interface"].astype(np.float64), axis=1)], axis=1)[:, :nz]
    w = wamp[:, None, :] * np.sin(np.pi * np.clip(zw / (0.75 * lid), 0.0, 1.0)) + rng.normal(0, 0.002, s3)
    qc = np.where(rng.random(s3) < 0.2, rng.uniform(0, 3e-4, s3), 0.0).astype(f32)
    qi = np.where(rng.random(s3) < 0.1, rng.uniform(0, 1e-4, s3), 0.0).astype(f32)
    if negzero:
        qc[ny // 2, 1, nx // 2] = f32(-0.0)
        qc[:, nz // 2, :] = f32(-0.0)                                        # a whole level: convective columns among them
        qi[1, 2, 0] = f32(-0.0)
    lm = c["land_mask"]
    if water:
        lm = np.where((np.arange(nx)[None, :] + np.arange(ny)[:, None]) % 3 == 0, 0, 2).astype(np.int32)
    zn = (np.arange(nz, 0, -1, dtype=np.float64) - 0.5) / nz                  # znu: half sigma levels, 1 at the ground to 0 at the top
    c.update(water_vapor=qv.astype(f32), w_real=w.astype(f32), cloud_water=qc, cloud_ice=qi, land_mask=lm, znu=zn.astype(f32),
             xland=np.where((lm == 0) | (lm == 2), 2.0, lm).astype(f32), negzero=bool(negzero))
    return c


def state(c):
    """what the calls carry: the four fields the tendencies are applied to, domain%temperature, and the results of the last call"""
    ny, nz, nx = c["density"].shape
    A = {k: np.ascontiguousarray(c[k], f32).copy() for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature")}
    for k in TEND:
        A[k] = np.zeros((ny, nz, nx), f32)
    for k in OUT2:
        A[k] = np.zeros((ny, nx), f32)
    A["ktype"] = np.zeros((ny, nx), np.int32)
    A["diag"] = np.zeros((ny, nx), np.int32)
    return A


def cu_tiedtke(c, A, dt, tile=None, kte=None, leveltop_col=0):
    """CU_TIEDTKE alone on the tile: the tendencies, RAINCV, PRATEC, KTYPE and the flags of A are written on the tile's columns"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or tile_of(c)
    ci = ctypes.c_int
    rc = lib().tiedtke_oracle_run(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ci(nz if kte is None else kte), ctypes.c_float(dt),
                                  _p(A["temperature"]), _p(A["water_vapor"]), _p(A["cloud_water"]), _p(A["cloud_ice"]), _p(c["exner"]),
                                  _p(c["density"]), _p(c["w_real"]), _p(c["dz_interface"]), _p(c["pressure"]), _p(c["pressure_interface"]),
                                  _p(c["xland"]), _p(c["znu"]), _p(A["tend_th"]), _p(A["tend_qv"]), _p(A["tend_qc"]), _p(A["tend_qi"]),
                                  _p(A["raincv"]), _p(A["pratec"]), _p(A["ktype"]), _p(A["diag"]), ci(leveltop_col))
    if rc:
        raise ValueError("tiedtke_oracle: level count refused")


def leveltop(c, its, j, kte=None):
    ny, nz, nx = c["density"].shape
    ci = ctypes.c_int
    return int(lib().tiedtke_oracle_leveltop(ci(nx), ci(nz), ci(ny), ci(its), ci(j), ci(nz if kte is None else kte), _p(c["pressure_interface"])))


def carry(c, A, dt):
    """the tendencies of the last call applied with every fraction 1 (cu_driver.f90:489-492), then domain%temperature as
    diagnostic_update makes it (T = theta exner)"""
    d = f32(dt)
    A["water_vapor"] = (A["water_vapor"] + A["tend_qv"] * d).astype(f32)
    A["cloud_water"] = (A["cloud_water"] + A["tend_qc"] * d).astype(f32)
    A["potential_temperature"] = (A["potential_temperature"] + A["tend_th"] * d).astype(f32)
    A["cloud_ice"] = (A["cloud_ice"] + A["tend_qi"] * d).astype(f32)
    A["temperature"] = (A["potential_temperature"] * c["exner"]).astype(f32)


def run_oracle(c, A, n, tile=None):
    """call n (0-based) of the carried sequence"""
    if n:
        carry(c, A, DT[n - 1])
    cu_tiedtke(c, A, DT[n], tile)


def fingerprint(c):
    return float(sum(float(np.asarray(c[k], np.float64).sum()) for k in INPUT3 + ["temperature", "potential_temperature", "water_vapor",
                                                                                   "cloud_water", "cloud_ice", "land_mask", "znu"]))


def convect(c, A, dt, tile=None, tendency_fraction=1.0, fractions=(1.0, 1.0, 1.0, 1.0)):
    """convect(domain, options, dt) (cu_driver.f90:255-514) with convection = kCU_TIEDTKE on the tile: the zeroing over all i and k of
    the rows jts..jte, CU_TIEDTKE, then x = x + tend dt fraction on those rows and the two precipitation sums; fractions: qv, qc, th, qi"""
    its, ite, jts, jte = tile or tile_of(c)
    rows = slice(jts - 1, jte)
    for k in TEND + ["raincv"]:
        A[k][rows] = 0
    cu_tiedtke(c, A, dt, (its, ite, jts, jte))
    d = f32(dt)
    if tendency_fraction > 0:
        for f, x, t in zip(fractions, ("water_vapor", "cloud_water", "potential_temperature", "cloud_ice"), ("tend_qv", "tend_qc", "tend_th", "tend_qi")):
            if f > 0:
                A[x][rows] = (A[x][rows] + A[t][rows] * d * f32(f)).astype(f32)
    A["accumulated_precipitation"][rows] = A["accumulated_precipitation"][rows] + A["raincv"][rows].astype(np.float64)
    A["accumulated_convective_pcp"][rows] = A["accumulated_convective_pcp"][rows] + A["raincv"][rows]


# ---- the same on the device -------------------------------------------------------------------------------------------------------
DEVICE_NAME = {"cloud_water": "cloud_water_mass", "cloud_ice": "cloud_ice_mass"}


def options_of(c, tendency_fraction=1.0, fractions=(-1.0, -1.0, -1.0, -1.0)):
    from icar_amd.options import options_t
    opt = options_t()
    opt.physics.convection = kCU_TIEDTKE
    opt.physics.advection = opt.physics.microphysics = 0
    o = opt.cu_options
    o.tendency_fraction = tendency_fraction
    o.tend_qv_fraction, o.tend_qc_fraction, o.tend_th_fraction, o.tend_qi_fraction = fractions
    return opt


def device_domain(c, grid=None, **kw):
    """a single-image domain_t holding the case (znu from the case), the slot initialised for kCU_TIEDTKE"""
    from util import single_image_domain
    from icar_amd import convection
    from icar_amd.domain import domain_t
    if grid is None:
        d = single_image_domain(c)
    else:
        d = domain_t(grid, device=0, dx=float(c["dx"]))
        d.load_case(c)
    d._cu_opt = options_of(c, **kw)
    convection.init_convection(d, d._cu_opt)
    d.fill("accumulated_precipitation", 0.0)
    return d


def device_put(d, A):
    """the carried fields of a host state to the device"""
    for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature"):
        d.set(DEVICE_NAME.get(k, k), A[k])


def device_state(d):
    from icar_amd import convection
    out = {"tend_th": convection.cu_get(d, "tend_th"), "tend_qv": convection.cu_get(d, "tend_qv"), "raincv": convection.cu_get(d, "raincv"),
           "accumulated_convective_pcp": convection.cu_get(d, "accumulated_convective_pcp")}
    out.update({k: convection.tiedtke_get(d, k) for k in ("tend_qc", "tend_qi", "pratec", "ktype")})
    out.update({k: d.get(DEVICE_NAME.get(k, k)) for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "accumulated_precipitation")})
    return out

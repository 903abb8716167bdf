"""TEST INFRASTRUCTURE: loader of tests/support/ysu_oracle.c (the CPU restatement of the boundary-layer slot with boundarylayer =
kPBL_YSU: the product's own header icar_amd/csrc/ysu_column.h compiled for the host, pbl_init's arrays, the driver's statements
around da_sfc_wtq and ysu) and the recipe of the YSU test cases.  The library is compiled with gcc -O2 -ffp-contract=off on first
use and by __graft_entry__.build(), so that it exists where the GPU tests run."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "ysu_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "ysu_column.h")
LIB = os.path.join(HERE, "support", "libysu_oracle.so")
f32 = np.float32
kPBL_YSU = 3
STATE3 = ["potential_temperature", "water_vapor", "cloud_water", "cloud_ice"]
TEND = ["tend_th", "tend_qv", "tend_qc", "tend_qi", "tend_u", "tend_v"]
OUT2 = ["hpbl", "kpbl", "hol", "psim", "psih", "regime", "ri", "windspd"]
INIT2 = ["z_atm", "gz1oz0", "zol", "hol"]
INPUT3 = ["u_mass", "v_mass", "pressure", "pressure_interface", "exner", "dz_interface", "z"]
INPUT2 = ["terrain", "roughness_z0", "surface_pressure", "skin_temperature", "ground_surf_temperature", "sensible_heat", "latent_heat",
          "u_10m", "v_10m", "ustar"]
# ysu_column's flags (icar_amd/csrc/ysu_column.h: YSU_D_*, YSU_C_*)
D_BELOW, D_FREE, D_MOIST, D_RI_NEG, D_ENTRAIN, D_KH_MIN, D_KH_MAX, D_KM_MIN, D_KM_MAX, D_PR_MIN, D_PR_MAX = (1 << n for n in range(11))
C_SFCFLG, C_PBLFLG, C_GAMCRT, C_GAMCRQ, C_RIMIN = (1 << n for n in range(5))
_lib = None


def build(force=False):
    if force or not os.path.exists(LIB) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(LIB):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", LIB, "-lm"])
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


MIN_NZ = lambda: int(lib().ysu_oracle_min_levels()) + 1      # model levels kts..kte: the scheme runs on kts..kte-1
MAX_NZ = lambda: int(lib().ysu_oracle_max_levels()) + 1

# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_ysu.py) and of the GPU tests --------------------------------
CASES = {"ysu_a_mixed_32x24x14": dict(nx=32, ny=24, nz=14, seed=1, lid=5000.0, water=0.35),
         "ysu_b_3lev_26x14x3": dict(nx=26, ny=14, nz=3, seed=2, lid=1500.0, water=0.2),
         "ysu_c_64lev_land_20x12x64": dict(nx=20, ny=12, nz=64, seed=3, lid=7000.0, water=0.0),
         "ysu_d_90lev_20x10x90": dict(nx=20, ny=10, nz=90, seed=4, lid=16000.0, water=0.3),
         "ysu_e_calm_negzero_30x20x24": dict(nx=30, ny=20, nz=24, seed=5, lid=0.0, water=0.3, calm=0.3, negzero=True),
         "ysu_f_deep_34x10x20": dict(nx=34, ny=10, nz=20, seed=6, lid=9000.0, water=0.1, hot=True)}
EXTRA_SEEDS = {"ysu_x_seed7_24x12x12": dict(nx=24, ny=12, nz=12, seed=7, lid=4000.0, water=0.4),
               "ysu_y_seed8_22x10x30": dict(nx=22, ny=10, nz=30, seed=8, lid=8000.0, water=0.15, calm=0.1)}
CALLS = 2
DT = (30.0, 75.0)


def make_case(nx, ny, nz, seed, lid=5000.0, water=0.3, calm=0.0, hot=False, negzero=False, regime3=0.04):
    """The probe state of the boundary-layer slot.  Layers: thickness growing with height up to `lid` (lid = 0: a stretched grid from a
    2.5 m lowest layer, factor 1.25, capped at 600 m).  A mixed layer of 150 m .. 2.5 km (hot: .. 5 km) under an inversion and a stable
    free atmosphere with some unstable kinks; the rows of the upper 45 % of j carry a surface inversion and a cold skin instead
    (stable columns).  Cloud slabs in a third of the columns, wind growing with height with a turning and sheared layers, `calm`: that
    share of the cells has no wind at 10 m at all.  Surface fluxes up to 600 W/m2 (hot: 1000), roughness 2 cm .. 0.8 m over land and
    0.1 .. 1 mm over the `water` share of the cells.  In a share regime3 of the cells the ground temperature is set to the REAL(4) at
    which da_sfc_wtq's bulk Richardson number is exactly zero (found by bisection on the restatement).  Everything in FP64, rounded
    once to REAL(4); the diagnostics are those diagnostic_update would leave."""
    rng = np.random.default_rng(7000 + seed)
    s3, s2 = (ny, nz, nx), (ny, nx)
    Rd, g, cp = 287.058, 9.81, 1012.0
    if lid > 0:
        w = 0.4 + 1.6 * np.arange(nz) / nz
        dzl = lid * w / w.sum()
    else:
        dzl = np.minimum(2.5 * 1.25 ** np.arange(nz), 600.0)
    dz = np.broadcast_to(dzl[None, :, None], s3) * rng.uniform(0.985, 1.0, s3)
    zi = np.concatenate([np.zeros((ny, 1, nx)), np.cumsum(dz, axis=1)], axis=1)
    zagl = 0.5 * (zi[:, :-1] + zi[:, 1:])
    terrain = 100.0 + 900.0 * rng.random(s2)
    fi = (np.arange(nx) / max(nx - 1, 1))[None, :] + np.zeros(s2)
    fj = (np.arange(ny) / max(ny - 1, 1))[:, None] + np.zeros(s2)
    stable = fj > 0.55
    lm = np.where(rng.random(s2) < water, 2, 1).astype(np.int32)
    th0 = 285.0 + 18.0 * fi + rng.normal(0, 0.3, s2)
    zml = 150.0 + ((5000.0 if hot else 2500.0) - 150.0) * rng.random(s2) ** (0.7 if hot else 1.5)
    gamma = 0.0035 + 0.003 * rng.random(s2)
    jump = 0.5 + 2.5 * rng.random(s2)
    above = np.maximum(zagl - zml[:, None, :], 0.0)
    theta = th0[:, None, :] + gamma[:, None, :] * above + jump[:, None, :] * (above > 0) + 0.05 * zagl / 1000.0
    inv = 0.008 + 0.02 * rng.random(s2)
    theta_s = th0[:, None, :] + inv[:, None, :] * np.minimum(zagl, 400.0) + 0.004 * np.maximum(zagl - 400.0, 0.0)
    theta = np.where(stable[:, None, :], theta_s, theta)
    kink = rng.random(s3) < 0.12                                              # unstable kinks: a layer warmer than the one above it
    theta = theta + np.where(kink, rng.uniform(0.2, 0.9, s3), 0.0) + rng.normal(0, 0.02, s3)
    psfc = 101000.0 - 11.5 * terrain + 300.0 * rng.random(s2)
    T = theta.copy()
    for _ in range(4):                                                        # hydrostatic under T = theta exner
        pint = np.empty((ny, nz + 1, nx)); pint[:, 0] = psfc
        for k in range(nz):
            pint[:, k + 1] = pint[:, k] * np.exp(-g * dz[:, k] / (Rd * T[:, k]))
        p = np.sqrt(pint[:, :-1] * pint[:, 1:])
        T = theta * (p / 1e5) ** (Rd / cp)
    es = 610.78 * np.exp(17.2693882 * (T - 273.16) / (T - 35.86))
    qs = 0.622 * es / np.maximum(p - es, 1.0)
    rh = (0.35 + 0.5 * rng.random(s2))[:, None, :] * np.where(zagl < zml[:, None, :], 1.0, np.exp(-(zagl - zml[:, None, :]) / 2500.0))
    qv = np.maximum(rh * qs, 1e-7)
    cloudy = (rng.random(s2) < 0.35)[:, None, :]
    zc = (300.0 + 2500.0 * rng.random(s2))[:, None, :]
    slab = cloudy & (zagl > zc) & (zagl < zc + 400.0 + 0.25 * (lid if lid > 0 else 3000.0))
    qc = np.where(slab & (T > 255.0), rng.uniform(0.3e-4, 4e-4, s3), 0.0)
    qc = np.where(rng.random(s3) < 0.03, rng.uniform(0, 2e-5, s3), qc)        # isolated wisps: one level of a pair alone
    qi = np.where(slab & (T < 268.0), rng.uniform(0.2e-4, 2e-4, s3), 0.0)
    spd0 = 0.3 + 14.0 * rng.random(s2) ** 1.5
    direction = 2 * np.pi * rng.random(s2)
    z0 = np.where(lm == 2, 1e-4 + 9e-4 * rng.random(s2), 0.02 + 0.78 * rng.random(s2) ** 2)
    prof = np.log(np.maximum(zagl, 1.0) / z0[:, None, :] + 1.0) / np.log(1000.0 / z0[:, None, :] + 1.0)
    turn = direction[:, None, :] + 0.3 * zagl / 2000.0
    shear = np.cumsum(np.where(rng.random(s3) < 0.15, rng.normal(0, 2.5, s3), rng.normal(0, 0.15, s3)), axis=1)
    um = spd0[:, None, :] * prof * np.cos(turn) + shear
    vm = spd0[:, None, :] * prof * np.sin(turn) + 0.5 * shear
    z1 = zagl[:, 0]
    lastw = np.log(10.0 / z0) / np.log(z1 / z0 + 1.0)
    u10, v10 = um[:, 0] * lastw, vm[:, 0] * lastw
    ustar = np.maximum(0.41 * np.hypot(um[:, 0], vm[:, 0]) / np.log(z1 / z0 + 1.0), 0.03)
    if calm > 0:
        still = rng.random(s2) < calm
        u10 = np.where(still, 0.0, u10); v10 = np.where(still, 0.0, v10)
        um[:, 0] = np.where(still, 0.02 * um[:, 0], um[:, 0]); vm[:, 0] = np.where(still, 0.02 * vm[:, 0], vm[:, 0])
        ustar = np.where(still, 0.03 + 0.05 * rng.random(s2), ustar)
    dts = np.where(stable, -(0.5 + 7.0 * rng.random(s2)), 0.5 + 9.0 * rng.random(s2) ** 1.3)
    near = rng.random(s2) < 0.25                                              # near-neutral cells: the regimes 2 and 4 of weak forcing
    dts = np.where(near, rng.normal(0, 0.15, s2), dts)
    tsk = T[:, 0] + dts
    tg = tsk + rng.normal(0, 0.4, s2)
    hfx = np.where(stable, -(3.0 + 60.0 * rng.random(s2)), 15.0 + ((1000.0 if hot else 600.0) - 15.0) * rng.random(s2) ** (0.6 if hot else 1.4))
    hfx = np.where(near, rng.normal(0, 8.0, s2), hfx)
    lh = np.where(stable, 20.0 * rng.random(s2) - 5.0, 10.0 + 440.0 * rng.random(s2) ** 1.2)
    lh = np.where((lm == 2) & ~stable, 150.0 + 450.0 * rng.random(s2), lh)
    p4, T4 = p.astype(f32), T.astype(f32)
    exner = ((p4.astype(np.float64) / 1e5) ** (Rd / cp)).astype(f32)
    c = dict(nx=nx, ny=ny, nz=nz, dx=f32(2000.0), dz_interface=dz.astype(f32), z=(zagl + terrain[:, None, :]).astype(f32), pressure=p4,
             pressure_interface=np.ascontiguousarray(pint[:, :nz]).astype(f32), temperature=T4, exner=exner,
             potential_temperature=(T4 / exner).astype(f32), density=(p4 / (f32(Rd) * T4)).astype(f32), water_vapor=qv.astype(f32),
             cloud_water=qc.astype(f32), cloud_ice=qi.astype(f32), u_mass=um.astype(f32), v_mass=vm.astype(f32), land_mask=lm,
             terrain=terrain.astype(f32), roughness_z0=z0.astype(f32), surface_pressure=psfc.astype(f32), skin_temperature=tsk.astype(f32),
             ground_surf_temperature=tg.astype(f32), sensible_heat=hfx.astype(f32), latent_heat=lh.astype(f32), u_10m=u10.astype(f32),
             v_10m=v10.astype(f32), ustar=ustar.astype(f32), negzero=bool(negzero))
    if negzero:
        c["cloud_water"][ny // 2, 1, nx // 2] = f32(-0.0)                     # inside the tile
        c["cloud_water"][1, 2, 0] = f32(-0.0)                                 # owned row, halo column
        c["cloud_water"][0, nz - 1, 3] = f32(-0.0)                            # halo row, the top level
    if regime3 > 0:
        pick = rng.random(s2) < regime3
        c["ground_surf_temperature"] = neutral_ground(c, pick)
    return c


def neutral_ground(c, pick):
    """ground_surf_temperature with, in the picked cells, the REAL(4) value at which da_sfc_wtq's rib is exactly 0 (regime 3) where
    one exists: bisection over the bit patterns of tg on the restatement's regime (4 = the ground too warm, 1 / 2 = too cold)"""
    tg = c["ground_surf_temperature"].copy()
    lo = np.full(tg.shape, f32(200.0)).view(np.int32).copy()
    hi = np.full(tg.shape, f32(360.0)).view(np.int32).copy()
    init = init_arrays(c)
    for _ in range(34):
        mid = ((lo.astype(np.int64) + hi) // 2).astype(np.int32)
        trial = np.where(pick, mid.view(f32), tg).astype(f32)
        r = sfc(dict(c, ground_surf_temperature=trial), init, c["temperature"], c["cloud_water"])["regime"]
        warm = r > 3.5
        exact = np.abs(r - 3.1) < 0.01
        hi = np.where(pick & (warm | exact), mid, hi)
        lo = np.where(pick & ~warm & ~exact, mid, lo)
    trial = np.where(pick, hi.view(f32), tg).astype(f32)
    r = sfc(dict(c, ground_surf_temperature=trial), init, c["temperature"], c["cloud_water"])["regime"]
    return np.where(pick & (np.abs(r - 3.1) < 0.01), trial, tg).astype(f32)


def init_arrays(c):
    """pbl_init's z_atm, gz1oz0, zol, hol (pbl_driver.f90:136-151)"""
    ny, nz, nx = c["z"].shape
    out = {k: np.zeros((ny, nx), f32) for k in INIT2}
    ci = ctypes.c_int
    lib().ysu_oracle_init(ci(nx), ci(nz), ci(ny), _p(c["z"]), _p(c["terrain"]), _p(c["roughness_z0"]), _p(out["z_atm"]), _p(out["gz1oz0"]),
                          _p(out["zol"]), _p(out["hol"]))
    return out


def sfc(c, init, temperature, cloud_water):
    """pbl_driver.f90:227-254: windspd, Ri, psim, psih, regime over the memory"""
    ny, nz, nx = c["z"].shape
    out = {k: np.zeros((ny, nx), f32) for k in ("windspd", "ri", "psim", "psih", "regime")}
    ci = ctypes.c_int
    lib().ysu_oracle_sfc(ci(nx), ci(nz), ci(ny), ctypes.c_float(float(c["dx"])), _p(c["u_10m"]), _p(c["v_10m"]), _p(temperature),
                         _p(c["skin_temperature"]), _p(init["z_atm"]), _p(c["surface_pressure"]), _p(c["ground_surf_temperature"]),
                         _p(c["pressure"]), _p(cloud_water), _p(c["u_mass"]), _p(c["v_mass"]), _p(c["roughness_z0"]), _p(c["land_mask"]),
                         _p(c["ustar"]), _p(out["windspd"]), _p(out["ri"]), _p(out["psim"]), _p(out["psih"]), _p(out["regime"]))
    return out


def state(c):
    """what the slot carries from call to call: the four scalars, temperature, the six tendencies, pbl_init's arrays, the results"""
    ny, nz, nx = c["z"].shape
    A = {k: np.ascontiguousarray(c[k], f32).copy() for k in STATE3 + ["temperature"]}
    for k in TEND + ["exch_h"]:
        A[k] = np.zeros((ny, nz, nx), f32)
    A.update(init_arrays(c))
    A["hpbl"] = np.zeros((ny, nx), f32); A["kpbl"] = np.zeros((ny, nx), np.int32)
    for k in ("psim", "psih", "regime", "ri", "windspd"):
        A[k] = np.zeros((ny, nx), f32)
    return A


def tile_of(c):
    ny, nz, nx = c["z"].shape
    return (2, nx - 1, 2, ny - 1) if nx > 3 and ny > 3 else (1, nx, 1, ny)


def run_sfc(c, A):
    A.update(sfc(c, A, A["temperature"], A["cloud_water"]))


def run_ysu(c, A, dt, tile=None, kte=None, diag=False):
    """call ysu(...) alone on the tile (the tendencies stay); returns ysu_column's flags (ny, nz, nx) when diag"""
    ny, nz, nx = c["z"].shape
    its, ite, jts, jte = tile or tile_of(c)
    dg = np.zeros((ny, nz, nx), np.int32) if diag else None
    ci = ctypes.c_int
    rc = lib().ysu_oracle_ysu(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ci(nz if kte is None else kte), ctypes.c_float(dt),
                              _p(c["u_mass"]), _p(c["v_mass"]), _p(A["temperature"]), _p(A["water_vapor"]), _p(A["cloud_water"]),
                              _p(A["cloud_ice"]), _p(c["pressure"]), _p(c["pressure_interface"]), _p(c["exner"]), _p(c["dz_interface"]),
                              _p(c["surface_pressure"]), _p(c["roughness_z0"]), _p(c["ustar"]), _p(c["land_mask"]), _p(c["sensible_heat"]),
                              _p(c["latent_heat"]), _p(c["skin_temperature"]), _p(A["gz1oz0"]), _p(A["windspd"]), _p(A["ri"]), _p(A["psim"]),
                              _p(A["psih"]), _p(c["u_10m"]), _p(c["v_10m"]), _p(A["tend_u"]), _p(A["tend_v"]), _p(A["tend_th"]), _p(A["tend_qv"]),
                              _p(A["tend_qc"]), _p(A["tend_qi"]), _p(A["exch_h"]), _p(A["hol"]), _p(A["hpbl"]), _p(A["kpbl"]), _p(dg))
    if rc:
        raise ValueError("ysu_oracle: level count refused")
    return dg


def run_apply(c, A, dt):
    ny, nz, nx = c["z"].shape
    ci = ctypes.c_int
    lib().ysu_oracle_apply(ci(nx), ci(nz), ci(ny), ctypes.c_float(dt), _p(A["water_vapor"]), _p(A["cloud_water"]), _p(A["potential_temperature"]),
                           _p(A["cloud_ice"]), _p(A["tend_u"]), _p(A["tend_v"]), _p(A["tend_th"]), _p(A["tend_qv"]), _p(A["tend_qc"]), _p(A["tend_qi"]))


def rediagnose(c, A):
    """what diagnostic_update does to domain%temperature in front of the next call (time_step.f90: T = theta exner)"""
    A["temperature"] = (A["potential_temperature"] * c["exner"]).astype(f32)


def run_oracle(c, A, n, tile=None, keep=None, kte=None):
    """call n (0-based) of the carried sequence: diagnostic_update's temperature (from the second call on), then pbl(domain, options,
    DT[n]).  keep (a dict): receives copies of the six tendencies and ysu_column's flags as they are between ysu and the update."""
    if n:
        rediagnose(c, A)
    run_sfc(c, A)
    dg = run_ysu(c, A, DT[n], tile, kte, diag=keep is not None)
    if keep is not None:
        keep.update({k: A[k].copy() for k in TEND})
        keep["diag"] = dg
    run_apply(c, A, DT[n])


def bitdiff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize == 4, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


def fingerprint(c):
    return float(sum(float(np.asarray(c[k], np.float64).sum()) for k in INPUT3 + INPUT2 + STATE3 + ["temperature", "land_mask"]))


def owned(c, a, tile=None):
    its, ite, jts, jte = tile or tile_of(c)
    return a[jts - 1:jte, ..., its - 1:ite]


# ---- the coverage conditions (tests/test_ysu_oracle.py; tests/golden/make_golden_ysu.py asserts them before it writes) ---------------
def coverage(c, A, keep, tile=None):
    """shares of the tile's columns / half levels on each side of ysu2d's branches after one call; regime, ri and kpbl are results the
    compiled reference's vectors hold too, the flags are ysu_column's own (the reference keeps them in locals)"""
    col = owned(c, keep["diag"][:, 0, :], tile)
    lev = owned(c, keep["diag"][:, 1:, :], tile)
    ri, kpbl, reg = owned(c, A["ri"], tile), owned(c, A["kpbl"], tile), A["regime"]
    pblflg = (col & C_PBLFLG) != 0
    sfcflg = (col & C_SFCFLG) != 0
    below, free = (lev & D_BELOW) != 0, (lev & D_FREE) != 0
    half = below | free
    share = lambda m, of: float(m[of].mean()) if of.any() else 0.0
    out = {"unstable": float((ri <= 0).mean()), "stable": float((ri > 0).mean()),
           "kpbl_distinct_with_pblflg": int(len(np.unique(kpbl[pblflg]))), "kpbl_is_1": float((kpbl == 1).mean()),
           "moist": share((lev & D_MOIST) != 0, free), "ri_neg": share((lev & D_RI_NEG) != 0, free),
           "entrain": share((lev & D_ENTRAIN) != 0, free & pblflg[:, None, :]),
           "xkzmin": share((lev & (D_KH_MIN | D_KM_MIN)) != 0, half), "xkzmax": share((lev & (D_KH_MAX | D_KM_MAX)) != 0, half),
           "prmin": share((lev & D_PR_MIN) != 0, half), "prmax": share((lev & D_PR_MAX) != 0, half),
           "gamcrt": share((col & C_GAMCRT) != 0, sfcflg), "gamcrq": share((col & C_GAMCRQ) != 0, sfcflg), "rimin": float(((col & C_RIMIN) != 0).mean())}
    for r in (1, 2, 3, 4):
        out[f"regime{r}"] = float((np.abs(reg - (r + 0.1)) < 0.01).mean())      # da_sfc_wtq runs over the whole memory
    return out


# ---- the same on the device -------------------------------------------------------------------------------------------------------
DEVICE_NAME = {"cloud_water": "cloud_water_mass", "cloud_ice": "cloud_ice_mass"}


def options_of(c):
    from icar_amd.options import options_t
    opt = options_t()
    opt.physics.boundarylayer = kPBL_YSU
    opt.physics.advection = opt.physics.microphysics = 0
    return opt


def device_domain(c, grid=None, init=True):
    """a single-image domain_t holding the case, pbl_init called with kPBL_YSU"""
    from util import single_image_domain
    from icar_amd import pbl
    from icar_amd.domain import domain_t
    if grid is None:
        d = single_image_domain(c)
    else:
        d = domain_t(grid, device=0, dx=float(c["dx"]))
        d.load_case(c)
    d._ysu_opt = options_of(c)
    if init:
        pbl.pbl_init(d, d._ysu_opt)
        pbl.ysu_set(d, "ground_surf_temperature", c["ground_surf_temperature"])
    return d


def device_call(d, c, n, dt=None):
    """call n of the carried sequence on the device: domain%temperature made again as diagnostic_update makes it (from the second
    call on), then icar_hip_pbl on the tile of the domain's grid"""
    from icar_amd import pbl
    if n:
        d.set("temperature", (d.get("potential_temperature") * c["exner"]).astype(f32))
    pbl.pbl(d, d._ysu_opt, DT[n] if dt is None else dt)


def device_state(d, names=None):
    from icar_amd import pbl
    out = {k: d.get(DEVICE_NAME.get(k, k)) for k in STATE3}
    for k in names or (TEND + ["exch_h"] + OUT2 + ["z_atm", "gz1oz0", "zol"]):
        out[k] = pbl.ysu_get(d, k)
    return out

"""TEST INFRASTRUCTURE: loader of tests/support/lsm_noah_driver_oracle.c (the CPU restatement of the Noah branch of lsm() around the call
of lsm_noah: the product's own cell header icar_amd/csrc/lsm_noah_driver_cell.h compiled for the host) and the recipe of its test cases.
The library is compiled with gcc -O2 -ffp-contract=off on first use; build(contract=True) makes the FMA-contracted variant that the
oracle test compares with.

A case is a Noah case of tests/noah_oracle.py (make_case: land, water and land-ice cells, the forcing of every carried call) plus what
lsm() reads around the call: the terrain and the first level's height, the 10 m winds of every call (calm cells among them), the
accumulated precipitation as a REAL(8) sum of the calls' amounts, and the model clock of every call -- one call of every case finds the
update gate shut.  CHS, Ri, QGH and current_precipitation of the Noah case's forcing are NOT used: lsm() computes them.  The tile is
the grid's: 2..nx-1, 2..ny-1 of the memory rectangle."""
import ctypes
import os
import subprocess

import numpy as np

import noah_oracle as N

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "lsm_noah_driver_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "lsm_noah_driver_cell.h")
LIB = os.path.join(HERE, "support", "liblsm_noah_driver_oracle.so")
LIB_FMA = os.path.join(HERE, "support", "liblsm_noah_driver_oracle_fma.so")
GOLDEN = os.path.join(HERE, "golden")
f32, f64 = np.float32, np.float64
_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
_libs = {}

# flags of lnd_oracle_pre / _post
PRE = {"ri_neg": 1, "ri_pos": 2, "chs_max": 4, "chs_min": 8, "wind0": 16, "land": 32, "cold": 64, "precip": 128}
POST = {"cqs2_small": 1, "chs2_small": 2, "qv_floor": 4, "tile": 8, "max_swe": 16}

# the Noah parameters are those of tests/noah_oracle.py's fixtures (so that round 21's coverage of SFLX carries over); closed: the
# 0-based call at which the gate is shut; max_swe: options%lsm_options%max_swe
CASES = {
    "lsm_noah_a_snowfall_melt_24x12": dict(noah="noah_a_snowfall_melt_24x12", seed=1, closed=2, max_swe=1e10),
    "lsm_noah_b_thaw_freeze_26x11": dict(noah="noah_b_thaw_freeze_26x11", seed=2, closed=3, max_swe=1e10),
    "lsm_noah_c_summer_rain_24x12": dict(noah="noah_c_summer_rain_24x12", seed=3, closed=1, max_swe=1e10),
    "lsm_noah_d_deep_pack_23x13": dict(noah="noah_d_deep_pack_23x13", seed=4, closed=2, max_swe=120.0),
    "lsm_noah_e_night_dew_25x12": dict(noah="noah_e_night_dew_25x12", seed=5, closed=4, max_swe=1e10),
}
SEEDS = {"seed_g": dict(noah="seed_g", seed=7, closed=1, max_swe=40.0), "seed_h": dict(noah="seed_h", seed=8, closed=2, max_swe=1e10)}

# what the block writes beside lsm_noah's outputs (N.OUT): (nx, ny) REAL(4), rainbl REAL(8)
DRV = ["chs", "rib", "qgh", "rainbl_step", "cqs2", "lnz", "base", "lwup", "rainbl8", "t2", "q2"]      # (snow, smstot, chs2 are in N.OUT)
WHOLE = ["snow", "smstot", "chs2"]                                                                   # of N.OUT, written over the whole memory rectangle
INIT = ["z0", "chs", "chs2", "rainbl_step", "rainbl8", "t2", "q2", "z_atm", "lnz", "base"]            # what the coupling writes


def build(force=False, contract=False):
    lib_ = LIB_FMA if contract else LIB
    if force or not os.path.exists(lib_) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(lib_):
        fp = ["-ffp-contract=fast", "-mfma"] if contract else ["-ffp-contract=off"]
        subprocess.check_call(["gcc", "-O2"] + fp + ["-fPIC", "-shared", SRC, "-o", lib_, "-lm"])
    return lib_


def lib(contract=False):
    if contract not in _libs:
        _libs[contract] = ctypes.CDLL(build(contract=contract))
    return _libs[contract]


def noah_params(p):
    return dict(N.CASES[p["noah"]] if p["noah"] in N.CASES else N.SEEDS[p["noah"]]) if isinstance(p["noah"], str) else dict(p["noah"])


def make_case(tab, noah, seed, closed, max_swe):
    q = noah_params(dict(noah=noah))
    c = N.make_case(tab, **q)
    rng = np.random.default_rng(22000 + seed)
    ny, nx = c["ny"], c["nx"]
    s2 = (ny, nx)
    ring = np.ones(s2, bool); ring[1:-1, 1:-1] = False
    c["terrain"] = rng.uniform(0.0, 800.0, s2).astype(f32)
    c["z1"] = (c["terrain"] + rng.uniform(12.0, 45.0, s2)).astype(f32)
    c["max_swe"] = f32(max_swe)
    c["closed"] = int(closed)
    c["update_interval"] = int(c["dt"])
    acc = rng.uniform(0.0, 3000.0, s2)                                         # a restart: rain has fallen already
    c["precip0"] = acc.copy()
    clock, now = [], 7200.0
    for n, F in enumerate(c["forcing"]):
        u = rng.normal(0.0, 2.5, s2); v = rng.normal(0.0, 2.5, s2)
        faint = rng.random(s2) < 0.05                                          # a breath of wind: |Ri| is huge
        u = np.where(faint, rng.uniform(0.004, 0.05, s2), u); v = np.where(faint, 0.0, v)
        calm = rng.random(s2) < 0.04
        u = np.where(calm | ring, 0.0, u); v = np.where(calm | ring, 0.0, v)    # u_10m / v_10m are 0 outside ims+1:ime-1, jms+1:jme-1
        F["u10"], F["v10"] = u.astype(f32), v.astype(f32)
        F["psfc"] = F["p8w1"].copy()
        acc = acc + F["rainbl"].astype(f64) * (1.0 + 1e-9 * rng.random(s2))     # a REAL(8) sum: the difference is not a REAL(4) number
        F["precip"] = acc.copy()
        now += float(c["dt"]) / 3.0 if n == closed else float(c["dt"]) * (1.0 if n % 2 == 0 else 1.5)
        clock.append(now)
    c["clock"] = clock
    c["noah_case"] = _noah_view(c)
    return c


def _noah_view(c):
    """the case as tests/noah_oracle.py's lsm_noah takes it: the forcing without what lsm() computes, no constant CQS2"""
    v = {k: x for k, x in c.items() if k not in ("forcing", "cqs2")}
    v["forcing"] = [{k: F[k] for k in ("qv", "p8w1", "p8w2", "t", "swdown", "glw")} for F in c["forcing"]]
    return v


def tile_of(c):
    return 2, c["nx"] - 1, 2, c["ny"] - 1


def state0(c):
    """N.state0 plus the arrays of the driver as domain_t / allocate_noah_data / lsm_init leave them"""
    s2 = (c["ny"], c["nx"])
    A = N.state0(c)
    A.update(qgh=np.full(s2, 0.02, f32), chs=np.zeros(s2, f32), rib=np.zeros(s2, f32), rainbl_step=np.zeros(s2, f32), cqs2=np.full(s2, 0.01, f32),
             t2=np.zeros(s2, f32), q2=np.zeros(s2, f32), lwup=np.zeros(s2, f32), rainbl8=np.zeros(s2, f64), z_atm=np.zeros(s2, f32),
             lnz=np.zeros(s2, f32), base=np.zeros(s2, f32), last_model_time=-999.0)
    A["rainbl"] = A["rainbl_step"]                                             # lsm_noah's name for current_precipitation
    return A


def lsm_init(tab, c, A, L=None):
    """lsm_init: the Noah part (N.lsm_init, on the whole memory as the device runs it) and the coupling"""
    L = L or lib()
    N.lsm_init(tab, c, A)
    F = c["forcing"][0]
    ci = ctypes.c_int
    L.lnd_oracle_couple(ci(c["nx"]), ci(c["ny"]), _p(A["znt"]), _p(c["z1"]), _p(c["terrain"]), _p(F["t"]), _p(F["qv"]), _p(c["precip0"]), _p(A["z0"]),
                        _p(A["chs"]), _p(A["chs2"]), _p(A["rainbl_step"]), _p(A["rainbl8"]), _p(A["t2"]), _p(A["q2"]), _p(A["z_atm"]), _p(A["lnz"]), _p(A["base"]))


def gate(c, A, now):
    """lsm_driver.f90:1016-1023: (open, lsm_dt)"""
    ui = float(c["update_interval"])
    if A["last_model_time"] == -999.0:
        A["last_model_time"] = now - ui
    if (now - A["last_model_time"]) >= ui:
        dt = f32(now - A["last_model_time"])
        A["last_model_time"] = now
        return True, float(dt)
    return False, 0.0


def pre(c, A, n, L=None):
    L = L or lib()
    F = c["forcing"][n]
    ci = ctypes.c_int
    fl = np.zeros((c["ny"], c["nx"]), np.int32)
    mask = np.ascontiguousarray(c["xland"], np.int32)
    L.lnd_oracle_pre(ci(c["nx"]), ci(c["ny"]), _p(F["u10"]), _p(F["v10"]), _p(A["tsk"]), _p(F["t"]), _p(A["z_atm"]), _p(A["lnz"]), _p(A["base"]), _p(A["t2"]),
                     _p(F["psfc"]), _p(mask), _p(F["precip"]), _p(A["rainbl8"]), _p(A["rib"]), _p(A["chs"]), _p(A["chs2"]), _p(A["cqs2"]), _p(A["qgh"]),
                     _p(A["rainbl_step"]), _p(fl))
    return fl


def post(c, A, n, tile=None, L=None):
    L = L or lib()
    F = c["forcing"][n]
    ci = ctypes.c_int
    its, ite, jts, jte = tile or tile_of(c)
    fl = np.zeros((c["ny"], c["nx"]), np.int32)
    L.lnd_oracle_post(ci(c["nx"]), ci(c["ny"]), ci(its), ci(ite), ci(jts), ci(jte), ctypes.c_float(float(c["max_swe"])), _p(A["z_atm"]), _p(A["znt"]),
                      _p(A["emiss"]), _p(A["tsk"]), _p(A["smois"]), _p(A["hfx"]), _p(A["qfx"]), _p(A["qsfc"]), _p(A["chs2"]), _p(A["cqs2"]), _p(F["psfc"]),
                      _p(F["precip"]), _p(A["snow"]), _p(A["lnz"]), _p(A["base"]), _p(A["lwup"]), _p(A["smstot"]), _p(A["t2"]), _p(A["q2"]), _p(A["rainbl8"]),
                      _p(fl))
    return fl


def lsm(tab, c, A, n, tile=None, L=None):
    """the gated block of lsm() at the clock of call n (watersurface 0 or 1: water_simple does not run); apply_fluxes is not part of
    this restatement (tests/sfc_oracle.py has it).  Returns (gate open, pre flags, post flags)."""
    is_open, dt = gate(c, A, c["clock"][n])
    if not is_open:
        return False, None, None
    pf = pre(c, A, n, L)
    N.lsm_noah(tab, c["noah_case"], A, n, tile or tile_of(c), dt)
    return True, pf, post(c, A, n, tile, L)


def shares(c, flags):
    """the coverage table from [(pre flags, post flags) of every open call]: name -> the largest share over the calls, of the tile's
    cells (wind0: a count)"""
    its, ite, jts, jte = tile_of(c)
    t = (slice(jts - 1, jte), slice(its - 1, ite))
    out = {}
    best = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), float(v)))
    for pf, qf in flags:
        p, q = pf[t], qf[t]
        land = p & PRE["land"] != 0
        best("ri_neg", (p & PRE["ri_neg"] != 0).mean()); best("ri_pos", (p & PRE["ri_pos"] != 0).mean())
        best("chs_max", (p & PRE["chs_max"] != 0).mean()); best("chs_min", (p & PRE["chs_min"] != 0).mean())
        best("chs_free", (p & (PRE["chs_max"] | PRE["chs_min"]) == 0).mean())
        best("sat_cold", (land & (p & PRE["cold"] != 0)).mean()); best("sat_warm", (land & (p & PRE["cold"] == 0)).mean())
        best("precip", (p & PRE["precip"] != 0).mean()); best("no_precip", (p & PRE["precip"] == 0).mean())
        best("wind0", (p & PRE["wind0"] != 0).sum())
        best("max_swe", (q & POST["max_swe"] != 0).mean()); best("qv_floor", (q & POST["qv_floor"] != 0).mean())
        best("cqs2_small", (q & POST["cqs2_small"] != 0).mean()); best("chs2_small", (q & POST["chs2_small"] != 0).mean())
        best("cqs2_large", (q & POST["cqs2_small"] == 0).mean()); best("chs2_large", (q & POST["chs2_small"] == 0).mean())
    return out


# each arm in at least 2 % of the tile's cells of some fixture; NOT_REACHED: the README says why
REQUIRED = ["ri_neg", "ri_pos", "chs_max", "chs_min", "chs_free", "sat_cold", "sat_warm", "precip", "no_precip", "max_swe", "qv_floor",
            "cqs2_large", "chs2_large"]
NOT_REACHED = ["cqs2_small", "chs2_small"]


def fingerprint(c):
    s = N.fingerprint(c["noah_case"])
    s += sum(float(np.asarray(c[k], f64).sum()) for k in ("terrain", "z1", "precip0")) + sum(c["clock"])
    return s + sum(float(np.asarray(F[k], f64).sum()) for F in c["forcing"] for k in ("u10", "v10", "precip"))


def bitdiff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = np.uint64 if a.dtype == f64 else np.uint32
    return int((a.view(v) != b.view(v)).sum())


# ---- the same on the device -------------------------------------------------------------------------------------------------------
LSM_OF = {"t2": "temperature_2m", "q2": "humidity_2m", "lwup": "longwave_up", "rainbl8": "rainbl", "z_atm": "z_atm", "lnz": "lnz_atm_term",
          "base": "base_exchange_term"}
NOAH_OF = dict(N.NOAH_OF, rainbl_step="current_precipitation")


def device_get(d, k):
    from icar_amd import surface
    if k in LSM_OF:
        return surface.lsm_get(d, LSM_OF[k])
    if k in N.FIELD_OF:
        return d.get(N.FIELD_OF[k])
    return surface.noah_get(d, NOAH_OF[k])


def options_of(c, watersurface=0):
    opt = N.options_of(c)
    opt.physics.watersurface = watersurface
    o = opt.lsm_options
    o.update_interval, o.max_swe = int(c["update_interval"]), float(c["max_swe"])
    o.sh_feedback_fraction, o.lh_feedback_fraction, o.sfc_layer_thickness = 0.625, 1.0, 30.0
    return opt


def atmosphere(c, nz=2):
    """the 3-D fields apply_fluxes needs beside lsm_noah's, constant in time: a first level thicker than sfc_layer_thickness (nz = 0)"""
    rng = np.random.default_rng(23000 + int(c["nx"]) * 100 + int(c["ny"]))
    s3 = (c["ny"], nz, c["nx"])
    return dict(dz_interface=np.full(s3, 60.0, f32), density=rng.uniform(0.9, 1.25, s3).astype(f32), exner=rng.uniform(0.9, 1.0, s3).astype(f32),
                potential_temperature=rng.uniform(270.0, 300.0, s3).astype(f32))


def device_forcing(d, c, n, win=None):
    """what the atmosphere and the host hand lsm() at call n: level-1 fields, radiation, surface pressure, the 10 m winds and the
    accumulated precipitation.  Neither CHS, Ri, QGH nor current_precipitation."""
    F = c["forcing"][n]
    cut = (lambda a: a) if win is None else (lambda a: a[win[0]][..., win[1]])
    two = lambda a, b: np.ascontiguousarray(np.stack([cut(a)] + [cut(b)] * (d.nz - 1), axis=1))      # (the levels above the second are not read)
    d.set("water_vapor", two(F["qv"], F["qv"]))
    d.set("temperature", two(F["t"], F["t"]))
    d.set("pressure_interface", two(F["p8w1"], F["p8w2"]))
    d.set("shortwave", cut(F["swdown"])); d.set("longwave", cut(F["glw"]))
    d.set("surface_pressure", cut(F["psfc"])); d.set("u_10m", cut(F["u10"])); d.set("v_10m", cut(F["v10"]))
    d.set("accumulated_precipitation", cut(F["precip"]))


def device_domain(tab, c, grid=None, couple=True, watersurface=0):
    """N.device_domain (tables, the case before lsm_init, icar_hip_lsm_init) with the options of this case, the fields lsm() reads, and --
    couple -- icar_hip_lsm_noah_couple run with the first call's atmosphere on the device"""
    from icar_amd import surface
    d = N.device_domain(tab, c, grid=grid, init=False)
    win = d._noah_win
    cut = (lambda a: a) if win is None else (lambda a: a[win[0]][..., win[1]])
    d.set("terrain", cut(c["terrain"]))
    z = np.ascontiguousarray(np.stack([cut(c["z1"]) + f32(80.0 * k) for k in range(d.nz)], axis=1))
    d.set("z", z)
    for k, a in atmosphere(c, d.nz).items():
        d.set(k, np.ascontiguousarray(cut(a)))
    device_forcing(d, c, 0, win)
    d.set("accumulated_precipitation", cut(c["precip0"]))                    # lsm_init sees what has fallen before the first call
    d._lnd_opt = options_of(c, watersurface)
    surface.noah_init(d, d._lnd_opt, fndsnowh=c["fndsnowh"])
    if couple:
        surface.noah_couple(d)
    return d


def device_call(d, c, n, dt=30.0):
    """call n on the device: the clock, the forcing, icar_hip_lsm"""
    from icar_amd import surface
    d.model_time_seconds = c["clock"][n]
    device_forcing(d, c, n, d._noah_win)
    surface.lsm(d, d._lnd_opt, dt)

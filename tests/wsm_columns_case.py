"""Inputs and oracle-side runs of the column-height sweeps of WSM3 and WSM6 (tests/test_gpu_wsm_columns.py and
tests/test_gpu_wsm_fall.py on the device, tests/test_wsm_columns_inputs.py for what the inputs and the oracle alone must meet,
tests/test_oracle_wsm_columns.py for the oracle against the compiled reference on the same inputs).  Needs no GPU.

Every height the library accepts: 3 .. 64 levels for WSM3, 4 .. 64 for WSM6.  Up to 63 levels the semi-Lagrangian fall
(icar_amd/csrc/wsm_fall.h) runs one wave per column with the km + 1 interfaces on the lanes, at 64 one thread per column.  A height
runs two states: `warm` (heated so far that rain falls fast through every level, the model top included) and `cold` (snow,
and for WSM6 graupel, reach the ground).  Both are seeded at random in every level with every class the scheme carries, 35 % of
the cells empty, so that fall speeds of zero sit inside a shaft and the speed jumps between neighbouring levels; every seventh
column of the tile is empty (no hydrometeor at all: the fall's early return, beside columns of the same 16-column tile that
fall)."""
import numpy as np
from icar_amd import ideal
from mp_columns_case import DEPTH, level_thickness

WSM3_HEIGHTS = list(range(3, 65))
WSM6_HEIGHTS = list(range(4, 65))
HEIGHTS = {3: WSM3_HEIGHTS, 6: WSM6_HEIGHTS}
NX, NY = 85, 5                 # its .. ite = 2 .. 84: 83 = 5 x 16 + 3 columns (k_w6_fall_tile: five full tiles and one of three columns,
                               # i.e. three idle waves and a partial one) = 64 + 19 (WSM3's 64-column x blocks); three rows
TILE = 16                      # W6_TC / W3_TC: columns per LDS tile of the fall kernels
CALLS = 3
STATES = {"warm": dict(cool0=-45.0, cool=1.0, moist=1.6, seed=0), "cold": dict(cool0=30.0, cool=0.5, moist=1.3, seed=1)}
K3 = ["potential_temperature", "water_vapor", "cloud_water", "rain"]
K6 = K3 + ["cloud_ice", "snow", "graupel"]
KEYS = {3: K3, 6: K6}
# what mp_driver.f90 passes to both schemes (the values tests/test_gpu_wsm3.py and tests/test_gpu_wsm6.py use; [0] = dt)
ARGS18 = np.array([0, 9.81, 1012.0, 4 * np.float32(461.6), 287.058, 461.5, 273.15, np.float32(461.5) / np.float32(287.058) - np.float32(1),
                   np.float32(287.058) / np.float32(461.5), 1e-15, 2.85e6, 2.5e6, 3.5e5, 1.28, 1000.0, 4190.0, 2106.0, 610.78], np.float32)
SEED_AMOUNT = {"cloud_water": 5e-4, "rain": 3e-3, "cloud_ice": 5e-5, "snow": 1e-3, "graupel": 2e-3}


def wsm_dt(nk):
    """The fall works with minor steps of at most 180 s.  Every eighth height from 16 up takes 240 s = two minor loops of 120 s; the others one
    step of 90 .. 175 s, the longer the thicker the levels: rain of some g/kg (7 .. 9 m/s) then falls 0.6 .. 1.6 km, more than one level
    wherever a level is thinner than that (mean thickness DEPTH / nk: from 9 levels up, and through the thin levels of shorter columns)"""
    if nk % 8 == 0 and nk >= 16:
        return 240.0
    return float(np.clip(0.5 * DEPTH / nk, 90.0, 175.0))


TOP_LEVEL = 100.0              # metres


def wsm_thickness(nk):
    """level_thickness(nk) -- 0.6 .. 1.4 of DEPTH / nk, differing from level to level, the lowest the thinnest -- with a top level of
    100 m and the levels below stretched so that the column keeps its depth.  Snow aloft falls 1 .. 2 m/s, 120 .. 350 m in a minor step:
    only through a top level thinner than that does the arrival height of the top interface sink below a whole level (`exit intp`),
    which the 0.2 .. 2.6 km of level_thickness() never allow WSM3 (its qrs is snow wherever the air is below 0 C)."""
    t = level_thickness(nk).astype(np.float64)
    total = t.sum()
    t[-1] = TOP_LEVEL
    t[:-1] *= (total - TOP_LEVEL) / t[:-1].sum()
    return t.astype(np.float32)


def empty_columns(nx=NX):
    """0-based i of the columns that start without any hydrometeor"""
    return np.arange(nx)[(np.arange(nx) % 7) == 4]


def make_case(scheme, nk, state, nx=NX, ny=NY, thickness=None):
    s = STATES[state]
    c = ideal.make_case(nx, ny, nk, hill_height=800.0, noise=0.03, seed=100 * nk + s["seed"], cool=s["cool0"],
                        uniform_dz=wsm_thickness(nk) if thickness is None else thickness)
    c["water_vapor"] = (c["water_vapor"] * np.float32(s["moist"])).astype(np.float32)
    rng = np.random.default_rng(1000 * nk + 10 * scheme + s["seed"])
    c["w_real"] = (c["w"] + 0.3 * rng.standard_normal(c["w"].shape)).astype(np.float32)
    shape = c["water_vapor"].shape
    for n in KEYS[scheme][2:]:
        f = (SEED_AMOUNT[n] * rng.random(shape) ** 3).astype(np.float32)
        f[rng.random(shape) < 0.35] = 0.0
        f[:, :, empty_columns(nx)] = 0.0
        c[n] = f
    return c


def oracle_run(orc, scheme, c, dt, calls=CALLS, cool=None, state="warm", tile=None, levels=None, ref=None, tiles=None):
    """`calls` calls of the oracle (math mode 0) -- or, with ref = oracle.ref, of the compiled reference -- on the case, cooled between
    them.  tile = 1-based (its, ite, jts, jte), default 2 .. nx-1, 2 .. ny-1, or tiles = several of them per call; levels = 1-based (kts, kte),
    default all.
    Returns the fields of KEYS[scheme] and the REAL(8) sums acc_rain, acc_snow (and acc_graupel) of the calls' REAL(4) amounts."""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    cool = STATES[state]["cool"] if cool is None else cool
    kts, kte = levels or (1, nz)
    if scheme == 3 and kts != 1:
        # oracle/wsm3_oracle.c takes kts = 1 only (like the reference's fall(i,1)); the scheme reads and writes nothing outside
        # kts .. kte, so the same range is the column cut to those levels
        cut = {k: (np.ascontiguousarray(v[:, kts - 1:kte, :]) if isinstance(v, np.ndarray) and v.ndim == 3 and v.shape == (ny, nz, nx) else v) for k, v in c.items()}
        cut["nz"] = kte - kts + 1
        sub = oracle_run(orc, scheme, cut, dt, calls=calls, cool=cool, state=state, tile=tile, tiles=tiles, ref=ref)
        out = {}
        for k, v in sub.items():
            if k in KEYS[scheme]:
                out[k] = c[k].copy()
                if k == "potential_temperature":
                    for _ in range(calls):
                        out[k] -= np.float32(cool)
                out[k][:, kts - 1:kte, :] = v
            else:
                out[k] = v
        return out
    tiles = tiles or [tile or (2, nx - 1, 2, ny - 1)]
    B = {n: c[n].copy() for n in KEYS[scheme]}
    z2 = lambda: np.zeros((ny, nx), np.float32)
    acc = {n: np.zeros((ny, nx), np.float64) for n in (("rain", "snow") if scheme == 3 else ("rain", "snow", "graupel"))}
    a18 = ARGS18.copy(); a18[0] = dt
    if ref is None:
        orc.set_math_mode(0)
        (orc.wsm3_init if scheme == 3 else orc.wsm6_init)()
    for _ in range(calls):
        if scheme == 3:
            rb = dict(rain=z2(), rainncv=z2(), snow=z2(), snowncv=z2(), sr=z2())
            a = (B["potential_temperature"], B["water_vapor"], B["cloud_water"], B["rain"], c["w_real"], c["density"], c["exner"], c["pressure"], c["dz_mass"])
        else:
            rb = dict(rain=z2(), sr=z2(), snow=z2(), graupel=z2())
            a = (B["potential_temperature"], B["water_vapor"], B["cloud_water"], B["rain"], B["cloud_ice"], B["snow"], B["graupel"], c["density"],
                 c["exner"], c["pressure"], c["dz_mass"])
        for (its, ite, jts, jte) in tiles:
            if scheme == 3 and ref is None:
                assert orc.wsm3(*a, a18, *rb.values(), its, ite, jts, jte, kts, kte) == 0
            elif scheme == 3:
                ref.wsm3(*a, dt, *rb.values(), its, ite, jts, jte, kts, kte)
            elif ref is None:
                assert orc.wsm6(*a, a18, rb["rain"], rb["sr"], rb["snow"], rb["graupel"], its, ite, jts, jte, kts, kte) == 0
            else:
                ref.wsm6(*a, dt, rb["rain"], z2(), rb["sr"], rb["snow"], rb["graupel"], its, ite, jts, jte, kts, kte)
        for n in acc:
            acc[n] += rb[n]
        B["potential_temperature"] -= np.float32(cool)
    out = dict(B)
    out.update({"acc_" + n: a for n, a in acc.items()})
    return out


def counted(orc, fn):
    """fn() with the fall's branch counters on: (fn's result, {name: count})"""
    buf = np.zeros(len(orc.WSM_FALL_COUNTERS), np.int64)
    orc.wsm_fall_counters(buf)
    try:
        out = fn()
    finally:
        orc.wsm_fall_counters(None)
    return out, dict(zip(orc.WSM_FALL_COUNTERS, (int(x) for x in buf)))


def untouched(c, got, scheme, calls=CALLS, cool=0.0, tile=None, levels=None, tiles=None):
    """every cell outside its .. ite, jts .. jte, kts .. kte of every field still holds the input's bytes (the potential temperature:
    the input cooled `calls` times, which the caller does to the whole array), and the accumulators are 0 there"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    tiles = tiles or [tile or (2, nx - 1, 2, ny - 1)]
    kts, kte = levels or (1, nz)
    out = np.ones((ny, nz, nx), bool); ring = np.ones((ny, nx), bool)
    for (its, ite, jts, jte) in tiles:
        out[jts - 1:jte, kts - 1:kte, its - 1:ite] = False; ring[jts - 1:jte, its - 1:ite] = False
    for k in KEYS[scheme]:
        x = c[k].copy()
        if k == "potential_temperature":
            for _ in range(calls):
                x -= np.float32(cool)
        if not np.array_equal(got[k][out].view(np.int32), x[out].view(np.int32)):
            return False
    return all(not got[a][ring].any() for a in got if a.startswith("acc_"))


# ---- columns for the fall on its own (oracle.wsm_fall_column / the probe library's icar_probe_wsm_fall) --------------------------
def denfac_of(den):
    """sqrt(den0 / den) as both schemes form it (mp_wsm6.f90:438-446)"""
    tv = np.float32(1.0) / den.astype(np.float32)
    return np.sqrt((tv * np.float32(1.28)).astype(np.float32)).astype(np.float32)


def probe_speed(q1, q2, den, denfac, tk):
    """oracle/wsm6_oracle.c: probe_speed, on arrays (float32 operation by operation): the speed the departure wind is built with"""
    f = np.float32
    s = (q1 + (q2 + q2)).astype(f)
    return (((denfac * f(60.0)).astype(f) * np.sqrt(np.sqrt((s * den).astype(f)).astype(f)).astype(f)).astype(f) * (tk / f(273.0)).astype(f)).astype(f)


def scheme_columns(nk, count=24):
    """`count` columns of the WSM6 states of this height (at 3 levels too: WSM6 refuses that height, but make_case builds its seven
    fields at any): dicts of den, denfac, tk, dz, ww (km,) and rql (2, km) = den * (snow, graupel) -- or den * (rain, cloud ice):
    every second column"""
    cols = []
    for state in STATES:
        c = make_case(6, nk, state)
        t = (c["potential_temperature"] * c["exner"]).astype(np.float32)
        jj, ii = np.meshgrid(np.arange(1, NY - 1), np.arange(1, NX - 1), indexing="ij")
        pick = np.random.default_rng(nk).permutation(jj.size)[:count // 2]
        for n, p in enumerate(pick):
            j, i = int(jj.flat[p]), int(ii.flat[p])
            den = c["density"][j, :, i].copy()
            a, b = ("snow", "graupel") if n % 2 else ("rain", "cloud_ice")
            rql = np.stack([den * c[a][j, :, i], den * c[b][j, :, i]]).astype(np.float32)
            dfac = denfac_of(den)
            ww = probe_speed(c[a][j, :, i], c[b][j, :, i], den, dfac, t[j, :, i])
            cols.append(dict(den=den, denfac=dfac, tk=t[j, :, i].copy(), dz=c["dz_mass"][j, :, i].copy(), ww=ww, rql=rql, dt=wsm_dt(nk), name=f"{state}{n}"))
    return cols


def synthetic_columns(km):
    """columns built for the edges of the fall (see tests/test_gpu_wsm_fall.py); all have den*q >= 0"""
    f = np.float32
    k = np.arange(km)
    dz0 = (f(13000.0 / km) * (f(0.6) + f(0.2) * ((k * 3) % 5).astype(f))).astype(f)
    den = (f(1.2) * (f(1.0) - f(0.8) * k.astype(f) / f(km))).astype(f)
    tk = (f(290.0) - f(70.0) * k.astype(f) / f(km)).astype(f)
    base = dict(den=den, denfac=denfac_of(den), tk=tk, dz=dz0, dt=120.0)
    rng = np.random.default_rng(7000 + km)
    q = lambda: (den * f(2e-3) * rng.random(km).astype(f) ** 2).astype(f)
    zeros = np.zeros(km, f)
    cols = []

    def add(name, ww, r1, r2=None, **kw):
        d = dict(base); d.update(kw)
        d.update(name=name, ww=np.ascontiguousarray(ww, f), rql=np.stack([r1, zeros if r2 is None else r2]).astype(f))
        cols.append(d)
    w_of = lambda r: probe_speed((r / den).astype(f), zeros, den, base["denfac"], tk)
    add("all_zero", zeros, zeros)
    for name, lev in (("one_bottom", 0), ("one_middle", km // 2), ("one_top", km - 1)):
        r = zeros.copy(); r[lev] = den[lev] * f(3e-3)
        add(name, w_of(r), r)
        add(name + "_second_field", w_of(r), zeros, r)
    r = q(); w = w_of(r); w[1::3] = 0.0
    add("zero_speeds_in_shaft", w, r, q())
    r = q()
    add("limiter_every_level", (f(0.5) + f(3.0) * k.astype(f) * dz0 / f(120.0)).astype(f), r, q())
    w = np.where(k % 2 == 0, f(1.0), f(1.0) + f(2.0) * dz0 / f(120.0)).astype(f)
    add("limiter_alternating", w, q(), q())
    w = np.full(km, 2.0, f); w[-1] = f(2.0) + f(4.0) * dz0[-1] / f(120.0)
    add("limiter_top_only", w, q(), q())
    w = np.full(km, 6.0, f); w[0] = f(0.5)
    add("limiter_level0_only", w, q(), q())
    w = np.full(km, 3.0, f); w[km // 2:] = f(3.0) + f(0.2) * dz0[km // 2] / f(120.0)       # one trip whose lift does not reach the level below
    w[: km // 2] = f(3.0)
    add("limiter_trip_then_pass", w, q(), q())
    add("all_below_ground", np.full(km, 9.0, f), q(), q(), dt=float(3.0 * dz0.sum() / 9.0))
    add("tiny_dt", np.full(km, 2.0, f), q(), q(), dt=float(0.01 * dz0.min() / 2.0))        # every arrival height next to its interface
    w = np.zeros(km, f); w[km // 2:] = f(0.03) * dz0.min() / f(120.0)                        # too slow for the limiter; nothing at the ground
    r = q(); r[: km // 2] = 0.0
    add("slow_aloft", w, r, q() * (k >= km // 2))
    dzw = (f(20.0) * np.power(f(10.0), (f(3.0) * ((k * 7) % km).astype(f) / f(max(km - 1, 1))))).astype(f)    # 20 m .. 20 km
    add("dz_three_decades", np.full(km, 8.0, f), q(), q(), dz=dzw, dt=150.0)
    # km - 1 cells of 15 m over a thick one, all falling 15 (km - 2) - 7 m: interface km - 1 stays 8 m above the thick cell's top, so
    # that cell takes in the arrival cells 1 .. km - 1: km - 3 whole ones between kb = 1 and kt = km - 1, the most the remap allows
    # (kt is found among the interfaces below the top one, so kt <= km - 1 and kt - kb - 1 <= km - 3)
    thin = np.full(km, 15.0, f); thin[0] = f(15.0 * 4 * km)
    add("thin_over_thick", np.full(km, 10.0, f), q(), q(), dz=thin, dt=float((15.0 * (km - 2) - 7.0) / 10.0))
    thin2 = np.full(km, 15.0, f); thin2[km // 2] = f(15.0 * 4 * km)
    add("thin_over_thick_middle", np.full(km, 10.0, f), q(), q(), dz=thin2, dt=float(15.0 * km / 10.0 * 0.9))
    r = q(); r[::2] = 0.0
    add("sawtooth_content", np.full(km, 4.0, f), r, q())
    for c_ in cols:
        assert (c_["rql"] >= 0).all() and (c_["dz"] > 0).all() and np.isfinite(c_["ww"]).all(), c_["name"]
    return cols


def oracle_fall(orc, col, nf, iter):
    """the oracle's fall of one column with the probe speed: (den*q (nf, km), precip (nf,))"""
    return orc.wsm_fall_column(col["den"], col["denfac"], col["tk"], col["dz"], col["ww"], col["rql"][:nf], col["dt"], iter=iter, speed=1)

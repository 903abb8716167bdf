"""Inputs and oracle-side runs of the column-height sweeps of the microphysics (tests/test_gpu_mp_columns.py on the device,
tests/test_mp_columns_inputs.py for what the inputs and the oracle alone must meet).  Needs no GPU.

The launch layout of Thompson and of mp_simple is a function of the level count alone (icar_amd/csrc/column_comm.h:
thompson_launch_geometry(), block_comm_geometry()); launch_geometry() asks the product's own header through the probe library."""
import ctypes
import numpy as np
from icar_amd import ideal
from util import seed_layered_hydrometeors

LANE, PACK = 1, 2
KIND = {0: "refused", LANE: "lane", PACK: "pack"}
# every height from 1 to 130, and both ends of every row of the launch table above that
HEIGHTS = list(range(1, 131)) + [146, 147, 170, 171, 204, 205, 256, 257, 341, 342, 512, 513, 1024]
SIMPLE_HEIGHTS = HEIGHTS[1:]   # mp_simple's column is the whole context's, and a context holds at least two levels
SINGLE_LEVEL = 2               # nk = 1 for Thompson: kts = kte = this level (1-based) of a three-level tile
TOO_TALL = 1025
FIELDS = ["water_vapor", "cloud_water", "rain", "cloud_ice", "snow", "graupel", "ice_number", "rain_number", "potential_temperature"]
R1 = 1e-12                     # mp_thompson.f90: the smallest mass the scheme treats as present
CALLS, COOL, MOIST = 6, 2.0, 2.0
DEPTH = 13000.0                # metres of every column, whatever its level count (the ideal case's pressure formula ends near 25 km)


def launch_geometry(probe, nk):
    """(thompson kind, threads per block, columns per block, mp_simple threads per block, mp_simple columns per block)"""
    v = [ctypes.c_int() for _ in range(5)]
    assert probe.icar_probe_launch_geometry(int(nk), *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def launch_table(probe, nmax=1024):
    """[(first nk, last nk, (kind, nt, cpb))]: the runs of equal Thompson launches over nk = 1 .. nmax"""
    runs = []
    for nk in range(1, nmax + 1):
        g = launch_geometry(probe, nk)[:3]
        if runs and runs[-1][2] == g:
            runs[-1][1] = nk
        else:
            runs.append([nk, nk, g])
    return [tuple(r) for r in runs]


def thompson_dt(nk):
    """60 s where the levels are thin enough for the sedimentation to take several sub-steps; up to 600 s where they are kilometres
    thick, so that the sub-step counts still differ from column to column"""
    return float(np.clip(0.3 * DEPTH / nk, 60.0, 600.0))


def level_thickness(nk):
    """nk thicknesses that differ from level to level (0.6 .. 1.4 of DEPTH / nk: a level read from the wrong slot shows)"""
    return (np.float32(DEPTH / nk) * (np.float32(0.6) + np.float32(0.2) * ((np.arange(nk) * 3) % 5).astype(np.float32))).astype(np.float32)


def tile_shape(group):
    """(nx, ny) of a narrow tile for blocks of `group` columns along i (aligned to multiples of `group`): the processed columns
    1 .. nx-2 make a partial block at the start, two full blocks and a partial block at the end; three processed rows.  nx is no
    multiple of group, except for group = 2 (where a partial last block needs an even nx) and group = 1."""
    nx = 7 if group == 1 else 3 * group + group // 2 + 1
    if group > 1:
        assert (nx - 2) % group != group - 1 and (nx % group != 0 or group == 2)
    return nx, 5


def column_groups(kind, cpb, nx):
    """lists of the processed columns (0-based i) that share a block: aligned groups of cpb for the packed kernel, the four
    waves of a block for the lane kernel"""
    cols = np.arange(1, nx - 1)
    key = cols // cpb if kind == PACK else (cols - 1) // 4
    return [cols[key == g] for g in np.unique(key)]


def make_case(nk, nx, ny, species=("rain", "cloud_ice", "snow", "graupel"), hill=1000.0):
    c = ideal.make_case(nx, ny, nk, hill_height=hill, noise=0.01, uniform_dz=level_thickness(nk))
    c["water_vapor"] = (c["water_vapor"] * np.float32(MOIST)).astype(np.float32)
    return seed_layered_hydrometeors(c, species)


def thompson_case(probe, nk):
    kind, nt, cpb = launch_geometry(probe, nk)[:3]
    nx, ny = tile_shape(cpb if kind == PACK else 4)
    return make_case(3 if nk == 1 else nk, nx, ny)


def thompson_oracle_run(orc, c, dt, calls=CALLS, cool=COOL, tiles=None, diag=True, levels=None):
    """`calls` Thompson calls of the oracle (math mode 0) on the case, cooled by `cool` K between them as run_case does.
    tiles: 1-based (its, ite, jts, jte) to run in each call, default the one tile 2 .. nx-1, 2 .. ny-1.
    levels: the one level (1-based) to run as kts = kte, default all.
    Returns (fields + accumulators after the last call, [the plan record of each call])."""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    s = {k: c[k].copy() for k in FIELDS + ["exner", "pressure", "dz_mass"]}
    acc = {k: np.zeros((ny, nx), np.float64) for k in ("rain", "snow", "graupel")}
    plans = []
    orc.set_math_mode(0)
    for _ in range(calls):
        r = np.zeros((ny, nx), np.float32); rv = r.copy(); sn = r.copy(); gr = r.copy(); sr = r.copy()
        plan = np.zeros((ny, nx, orc.TH_DIAG_N), np.int32)
        orc.thompson_diag(plan if diag else None)
        try:
            for (its, ite, jts, jte) in (tiles or [(2, nx - 1, 2, ny - 1)]):
                orc.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"],
                             s["rain_number"], s["potential_temperature"], s["exner"], s["pressure"], s["dz_mass"], dt, r, rv, sn, gr, sr,
                             1, nx, 1, ny, 1, nz, its, ite, jts, jte, levels or 1, levels or nz)
        finally:
            orc.thompson_diag(None)
        plans.append(plan)
        acc["rain"] += r; acc["snow"] += sn; acc["graupel"] += gr
        s["potential_temperature"] -= np.float32(cool)
    ref = {k: s[k] for k in FIELDS}
    ref["acc_rain"] = acc["rain"]; ref["acc_snow"] = acc["snow"]; ref["acc_graupel"] = acc["graupel"]
    return ref, plans


def untouched(c, ref, calls=CALLS, cool=COOL):
    """the ring and the last global row and column of every field of ref still hold the input (the potential
    temperature: the input cooled `calls` times, which the test itself does to the whole array)"""
    ring = np.ones((c["ny"], c["nx"]), bool); ring[1:-1, 1:-1] = False
    for k in FIELDS:
        x = c[k].copy()
        if k == "potential_temperature":
            for _ in range(calls):
                x -= np.float32(cool)
        if not np.array_equal(ref[k].transpose(0, 2, 1)[ring].view(np.int32), x.transpose(0, 2, 1)[ring].view(np.int32)):
            return False
    return all(not ref[a][ring].any() for a in ("acc_rain", "acc_snow", "acc_graupel"))


def check_thompson_oracle(c, ref, plans, kind, cpb):
    """What the oracle alone must meet at a height before the device is compared with it (conditions on the inputs, not measurements):
    raises AssertionError naming the first that does not hold."""
    nk, nx = (1 if kind == LANE and c["nz"] == 3 else c["nz"]), c["nx"]
    for k, a in ref.items():
        assert np.isfinite(a).all(), f"{k}: not finite"
    if nk == 1:                                                                     # the single level of a three-level tile
        for k in FIELDS[:-1]:
            assert np.array_equal(ref[k][:, 0::2, :], c[k][:, 0::2, :]), f"{k}: a level outside kts .. kte changed"
    assert untouched(c, ref, len(plans)), "the ring or the last row / column changed"
    inner = (slice(1, -1), slice(None), slice(1, -1))
    if nk >= 8:
        for s in ("rain", "snow", "graupel", "cloud_ice"):
            assert ref[s][inner].max() > R1, f"no {s} after the last call"
        assert ref["acc_rain"].max() > 0, "no rain reached the surface"
        assert max(int(p[..., 4].max()) for p in plans) >= 2, "no fall speed was carried down over 2 or more levels"
        if nk >= 70:
            assert sum(int(p[..., 5].sum()) for p in plans) > 0, "no carried fall speed crosses level 63 / 64"
    else:
        for s in ("rain", "snow", "graupel", "cloud_ice", "water_vapor", "potential_temperature"):
            assert not np.array_equal(ref[s][inner], c[s][inner]), f"{s} did not change"
    if kind == PACK and cpb >= 2:
        # the largest sub-step count of a column against that of its block (plan4's nblk): two columns of one block differ
        differ = False
        for p in plans:
            nmax = p[..., :4].max(axis=-1)                                         # (ny, nx)
            for g in column_groups(kind, cpb, nx):
                differ |= bool((nmax[1:-1][:, g].max(axis=1) != nmax[1:-1][:, g].min(axis=1)).any())
        assert differ, "all columns of every block have the same largest sub-step count"


# ---- mp_simple ----------------------------------------------------------------------------------------------------------------
SIMPLE_IN = ["pressure", "potential_temperature", "exner", "density", "water_vapor", "cloud_water", "rain", "snow", "dz_mass"]
SIMPLE_OUT = {"potential_temperature": "potential_temperature", "water_vapor": "water_vapor", "cloud_water": "cloud_water_mass",
              "rain": "rain_mass", "snow": "snow_mass"}
SIMPLE_CALLS, SIMPLE_COOL = 4, 1.5


def simple_dt(nk):
    """a time step for which rain's Courant number in the thinnest level is 8.6 over flat ground: the Jacobian
    of simple_case's 3 km hill (0.77 .. 1) then makes the sub-step count ceil(dt / dz * 10) 9 .. 12 from column to column"""
    return float(np.float32(0.86 * 0.6 * DEPTH / nk))


def simple_case(probe, nk):
    cpb = launch_geometry(probe, nk)[4]
    nx, ny = tile_shape(cpb)
    return make_case(nk, nx, ny, species=("rain", "snow"), hill=3000.0)


def simple_ncfl(c, dt, top=None):
    """(rain, snow) sub-step counts per column as mp_simple.f90:503-562 computes them for columns that hold the species (float32)"""
    f32 = np.float32
    dz = c["dz_mass"]
    return tuple(np.ceil((f32(dt) / dz * f32(v)).max(axis=1)).astype(np.int32) for v in (10.0, 1.5))


def simple_oracle_run(orc, c, dt, calls=SIMPLE_CALLS, cool=SIMPLE_COOL, top=None, tiles=None):
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    s = {k: c[k].copy() for k in SIMPLE_IN}
    acc_r = np.zeros((ny, nx), np.float64); acc_s = np.zeros((ny, nx), np.float64)
    orc.set_math_mode(0)
    for _ in range(calls):
        rain = np.zeros((ny, nx), np.float32); snow = np.zeros((ny, nx), np.float32)
        for (its, ite, jts, jte) in (tiles or [(2, nx - 1, 2, ny - 1)]):
            err = orc.mp_simple(s["pressure"], s["potential_temperature"], s["exner"], s["density"], s["water_vapor"], s["cloud_water"],
                                s["rain"], s["snow"], rain, snow, dt, s["dz_mass"], its, ite, jts, jte, 1, nz if top is None else top)
            assert err == 0
        acc_r += rain; acc_s += snow
        s["potential_temperature"] -= np.float32(cool)
    ref = {k: s[k] for k in SIMPLE_OUT}
    ref["acc_rain"] = acc_r; ref["acc_snow"] = acc_s
    return ref


def check_simple_oracle(c, ref, dt, cpb):
    nx = c["nx"]
    for k, a in ref.items():
        assert np.isfinite(a).all(), f"{k}: not finite"
    inner = (slice(1, -1), slice(None), slice(1, -1))
    if c["nz"] >= 8:
        assert ref["rain"][inner].max() > 1e-30 and ref["snow"][inner].max() > 1e-30, "rain and snow must both be there after the last call"
    assert ref["acc_rain"].max() > 0, "nothing reached the surface"
    for k in ("rain", "snow", "water_vapor", "potential_temperature"):
        assert not np.array_equal(ref[k][inner], c[k][inner]), f"{k} did not change"
    if cpb >= 2:
        ncfl = simple_ncfl(c, dt)[0]
        differ = any((ncfl[1:-1][:, g].max(axis=1) != ncfl[1:-1][:, g].min(axis=1)).any() for g in column_groups(PACK, cpb, nx))
        assert differ, "rain's sub-step count is the same in all columns of every block"

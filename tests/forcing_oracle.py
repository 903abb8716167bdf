"""TEST INFRASTRUCTURE: loader of tests/support/forcing_oracle.c (the CPU restatement of the forcing update: the product's own header
icar_amd/csrc/forcing_interp.h compiled for the host), the chain interpolate_forcing / update_delta_fields assembled from it and from
oracle/wind_oracle.c's smooth_array, and the recipe of the forcing test cases.  The library is compiled with gcc -O2 -ffp-contract=off on
first use and by __graft_entry__.build(), so that it exists where the GPU tests run.

Arrays are numpy in C order == the reference's Fortran order read backwards: a model field (ny, nz, nx), a forcing variable
(ny_f, nz_f, nx_f), geolut x / y / w (ny, nx, 4), vert_lut z / w (ny, nz, nx, 2)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SRC = os.path.join(HERE, "support", "forcing_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "forcing_interp.h")
LIB = os.path.join(HERE, "support", "libforcing_oracle.so")
GOLDEN = os.path.join(HERE, "golden")
f32 = np.float32
D_STAY1, D_JUMP, D_EXIT, D_DZ_POS, D_DZ_NEG = 1, 2, 4, 8, 16      # forcing_interp.h: FI_D_*
FORCED = ["water_vapor", "potential_temperature", "pressure", "u", "v"]      # the forced set of every case, in this order
DT_SECONDS = 3600.0
_lib = None


def build(force=False, contract=False, out=None):
    out = out or LIB
    if force or not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(out):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-DFI_CONTRACT=%d" % int(contract), SRC, "-o", out, "-lm"])
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def bitdiff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def geo_vinterp(lo, G, L=None):
    """geo_interp + vinterp onto the grid of the tables G"""
    L = L or lib()
    ny, nz, nx, _ = G["z"].shape
    nyf, nzf, nxf = lo.shape
    out = np.empty((ny, nz, nx), f32)
    ci = ctypes.c_int
    L.fo_geo_vinterp(_p(lo), ci(nxf), ci(nzf), ci(nyf), _p(G["x"]), _p(G["y"]), _p(G["w"]), _p(G["z"]), _p(G["zw"]), ci(nx), ci(nz), ci(ny), _p(out))
    return out


def geo_novert(lo, G, nz, L=None):
    """geo_interp and the vert_interp = .false. branch; with nz = the forcing's level count it is geo_interp alone"""
    L = L or lib()
    ny, nx, _ = G["x"].shape
    nyf, nzf, nxf = lo.shape
    out = np.empty((ny, nz, nx), f32)
    ci = ctypes.c_int
    L.fo_geo_novert(_p(lo), ci(nxf), ci(nzf), ci(nyf), _p(G["x"]), _p(G["y"]), _p(G["w"]), ci(nx), ci(nz), ci(ny), _p(out))
    return out


def adjust_pressure(p_nv, th_nv, z_f, z_d, diag=None, L=None):
    L = L or lib()
    ny, nz, nx = p_nv.shape
    assert z_f.shape[1] >= nz and nz <= 1024
    out = np.empty_like(p_nv)
    ci = ctypes.c_int
    L.fo_adjust_pressure(_p(p_nv), _p(th_nv), _p(z_f), _p(z_d), _p(out), ci(nx), ci(nz), ci(z_f.shape[1]), ci(ny), _p(diag))
    return out


def smooth(a, w):
    """smooth_array(a, windowsize = w, ydim = 3) in place (oracle/wind_oracle.c)"""
    from oracle import orc
    orc.build()
    assert a.flags.c_contiguous and a.dtype == f32
    orc.smooth_array_ydim3(a, int(w))


def interp_wind(lo, G, nsmooth, shape, L=None):
    """interpolate_variable's u / v branch: lo is smoothed IN PLACE, as the reference smooths input_data%data_3d"""
    smooth(lo, 1)
    ext = geo_vinterp(lo, G, L)
    smooth(ext, nsmooth)
    ny, nz, nx = shape
    return np.ascontiguousarray(ext[G["j0"]:G["j0"] + ny, :, G["i0"]:G["i0"] + nx])


def interpolate_forcing(c, lo, out, diag=None, L=None, fields=None):
    """domain%interpolate_forcing: lo = {name: forcing array} (u, v are smoothed in place), out = {name: destination}, written in full"""
    ny, nz, nx = c["z"].shape
    for n in (FORCED if fields is None else fields):
        if n == "u":
            out[n] = interp_wind(lo[n], c["geo_u"], c["nsmooth"], (ny, nz, nx + 1), L)
        elif n == "v":
            out[n] = interp_wind(lo[n], c["geo_v"], c["nsmooth"], (ny + 1, nz, nx), L)
        elif n == "pressure":
            p_nv = geo_novert(lo[n], c["geo"], nz, L)
            th_nv = geo_novert(lo["potential_temperature"], c["geo"], nz, L)
            out[n] = adjust_pressure(p_nv, th_nv, c["geo_z"], c["z"], diag, L)
        else:
            out[n] = geo_vinterp(lo[n], c["geo"], L)


def update_delta(dqdt, data, dt, L=None, fields=None):
    L = L or lib()
    for n in list(FORCED if fields is None else fields) + ["w"]:
        assert dqdt[n].flags.c_contiguous and data[n].flags.c_contiguous and dqdt[n].shape == data[n].shape
        L.fo_delta(_p(dqdt[n]), _p(data[n]), ctypes.c_size_t(dqdt[n].size), ctypes.c_double(dt))


def run_oracle(c, L=None, diag=False):
    """the two carried forcing steps of a case over forced_of(c): (fields after step 1, dqdt after interpolate_forcing(update), dqdt
    after update_delta_fields, the forcing's u / v arrays as the two smoothings left them and step 2's pressure and potential
    temperature without vertical interpolation -- both arms of :2752-2760 --, adjust_pressure's flags of step 2)"""
    names = forced_of(c)
    lo1 = {n: c["lo1"][n].copy() for n in FORCED}
    lo2 = {n: c["lo2"][n].copy() for n in FORCED}
    data, dq = {}, {}
    interpolate_forcing(c, lo1, data, L=L, fields=names)
    data["w"] = c["w"].copy()
    dg = np.zeros(c["z"].shape, np.uint8) if diag and c["adjust"] else None
    interpolate_forcing(c, lo2, dq, dg, L=L, fields=names)
    dq["w"] = c["dqdt_w"].copy()
    pre = {n: dq[n].copy() for n in dq}
    update_delta(dq, data, DT_SECONDS, L=L, fields=names)
    nz = c["z"].shape[1]
    other = {"u1": lo1["u"], "v1": lo1["v"], "u2": lo2["u"], "v2": lo2["v"], "nv_pressure": geo_novert(lo2["pressure"], c["geo"], nz, L),
             "nv_theta": geo_novert(lo2["potential_temperature"], c["geo"], nz, L)}
    return data, pre, dq, other, dg


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_forcing.py) ---------------------------------------------------
# ext: cells by which the extended staggered grids reach beyond the tile to the west, east, south, north (domain_obj.f90:2177-2182 clips
# them at the domain's edge: 0 on a side that is one)
CASES = {
    "forcing_a_below_37x9x23": dict(nx=37, nz=9, ny=23, nxf=7, nzf=12, nyf=6, seed=1, nsmooth=2, ext=(2, 2, 2, 2), model_top=5500.0, forcing_top=14000.0,
                                    relief=900.0, first_f=180.0),
    "forcing_b_pad_30x14x20": dict(nx=30, nz=14, ny=20, nxf=6, nzf=6, nyf=5, seed=2, nsmooth=1, ext=(1, 1, 1, 1), model_top=9000.0, forcing_top=7000.0,
                                   relief=300.0, first_f=60.0, pressure=False),
    "forcing_c_top_24x8x16": dict(nx=24, nz=8, ny=16, nxf=9, nzf=8, nyf=7, seed=3, nsmooth=2, ext=(2, 2, 2, 2), model_top=16000.0, forcing_top=9000.0,
                                  relief=500.0, first_f=40.0),
    "forcing_d_shear_20x10x12": dict(nx=20, nz=10, ny=12, nxf=5, nzf=10, nyf=4, seed=4, nsmooth=1, ext=(1, 1, 1, 1), model_top=8000.0, forcing_top=12000.0,
                                     relief=600.0, first_f=120.0, shear=0.35, rot=-0.25, edge=True),
    "forcing_e_clip_26x7x18": dict(nx=26, nz=7, ny=18, nxf=8, nzf=9, nyf=7, seed=5, nsmooth=1, ext=(0, 1, 1, 0), model_top=6000.0, forcing_top=10000.0,
                                   relief=400.0, first_f=90.0),
    "forcing_f_wide_5x6x14": dict(nx=5, nz=6, ny=14, nxf=6, nzf=8, nyf=6, seed=6, nsmooth=3, ext=(3, 3, 3, 3), model_top=5000.0, forcing_top=9000.0,
                                  relief=200.0, first_f=70.0, negzero=True),
}
EXTRA_SEEDS = {
    "forcing_x_seed7_22x11x13": dict(nx=22, nz=11, ny=13, nxf=6, nzf=13, nyf=5, seed=7, nsmooth=2, ext=(2, 0, 0, 2), model_top=7000.0, forcing_top=11000.0,
                                     relief=700.0, first_f=150.0, shear=0.2),
    "forcing_y_seed8_18x12x15": dict(nx=18, nz=12, ny=15, nxf=7, nzf=12, nyf=6, seed=8, nsmooth=3, ext=(3, 3, 3, 3), model_top=12000.0, forcing_top=8000.0,
                                     relief=350.0, first_f=50.0, rot=0.15),
}


def _levels(n, first, top):
    """n mass-level heights above ground: the first at `first`, stretched geometrically up to `top`"""
    if n == 1:
        return np.array([first])
    return first * (top / first) ** (np.arange(n) / (n - 1))


def make_inputs(nx, nz, ny, nxf, nzf, nyf, seed, nsmooth, ext, model_top, forcing_top, relief, first_f, shear=0.0, rot=0.0, edge=False,
                negzero=False, pressure=True):
    """Everything of a case but the look-up tables: the coordinates geo_LUT and vLUT are made from, the forcing's arrays of two forcing
    steps, w and its dqdt.  The forcing grid is regular in a sheared / rotated (lon, lat); the model tile lies inside it (edge: the first
    column of the extended u grid and the first row of the extended v grid sit on the forcing grid's first column and row), every grid of the model is the same affine function of a continuous
    cell index.  FP64, rounded once to REAL(4).  pressure = False: the forcing has fewer levels than the model, which adjust_pressure
    cannot take (it reads forcing%geo%z out of bounds): the pressure is then interpolated without the adjustment."""
    rng = np.random.default_rng(9100 + seed)
    w_, e_, s_, n_ = ext
    # the tile in forcing-index space: cell ic of the model sits at a0 + ic sx
    lo_a, hi_a = (0.0 if edge else 0.75), nxf - 1.75
    lo_b, hi_b = (0.0 if edge else 0.75), nyf - 1.75
    sx = (hi_a - lo_a) / (nx + w_ + e_ + 2.0)
    sy = (hi_b - lo_b) / (ny + s_ + n_ + 2.0)
    a0 = lo_a + (w_ + (0.5 if edge else 1.0)) * sx               # edge: the first column of the extended u grid and the first row of
    b0 = lo_b + (s_ + (0.5 if edge else 1.0)) * sy               # the extended v grid sit on the forcing grid's first column / row
    dl = 0.5                                                     # degrees per forcing cell

    def lonlat(a, b):
        return 10.0 + dl * (a + shear * b), 45.0 + dl * (b + rot * a)

    def terrain_f(a, b):
        return 0.5 * relief * (1.0 + np.sin(1.3 * a + 0.4) * np.cos(0.9 * b - 0.2))

    def terrain_m(a, b):
        return np.maximum(terrain_f(a, b) + 0.45 * relief * np.sin(5.1 * a) * np.sin(4.3 * b + 1.0), 0.0)

    zf_lev = _levels(nzf, first_f, forcing_top)
    zm_lev = _levels(nz, 15.0, model_top)
    jf, if_ = np.meshgrid(np.arange(nyf, dtype=np.float64), np.arange(nxf, dtype=np.float64), indexing="ij")
    c = {"nsmooth": int(nsmooth)}
    c["lo_lon"], c["lo_lat"] = (v.astype(f32) for v in lonlat(if_, jf))
    c["lo_z"] = (terrain_f(if_, jf)[:, None, :] + zf_lev[None, :, None] * (1.0 + 0.03 * np.sin(if_ + jf))[:, None, :]).astype(f32)

    def grid(nxg, nyg, di, dj):
        jj, ii = np.meshgrid(np.arange(nyg, dtype=np.float64), np.arange(nxg, dtype=np.float64), indexing="ij")
        a, b = a0 + (ii + di) * sx, b0 + (jj + dj) * sy
        lon, lat = lonlat(a, b)
        z = terrain_m(a, b)[:, None, :] + zm_lev[None, :, None]
        return {"lon": lon.astype(f32), "lat": lat.astype(f32), "z": z.astype(f32)}

    c["hi"] = grid(nx, ny, 0.0, 0.0)
    c["hi_u"] = dict(grid(nx + 1 + w_ + e_, ny + s_ + n_, -0.5 - w_, -s_), i0=w_, j0=s_)
    c["hi_v"] = dict(grid(nx + w_ + e_, ny + 1 + s_ + n_, -w_, -0.5 - s_), i0=w_, j0=s_)
    c["z"] = c["hi"]["z"]
    sf = (nyf, nzf, nxf)
    zf = c["lo_z"].astype(np.float64)

    def forcing_fields(shift):
        th = 285.0 + shift + 0.004 * zf + rng.normal(0, 0.4, sf)
        p = 100500.0 * np.exp(-zf / (29.3 * 0.5 * (th + 285.0) * (1.0 - 0.00005 * zf))) * (1.0 + 0.002 * rng.standard_normal(sf))
        qv = 0.012 * np.exp(-zf / 2500.0) * rng.uniform(0.3, 1.0, sf)
        out = {"water_vapor": qv, "potential_temperature": th, "pressure": p, "u": 8.0 + shift + 6.0 * rng.standard_normal(sf),
               "v": -3.0 + 5.0 * rng.standard_normal(sf)}
        return {k: np.ascontiguousarray(v, f32) for k, v in out.items()}

    c["lo1"], c["lo2"] = forcing_fields(0.0), forcing_fields(1.5)
    if negzero:                                                   # a plane of -0.0 in qv: every sum that starts from 0 gives +0
        for lo in (c["lo1"], c["lo2"]):
            lo["water_vapor"][:, 1, :] = f32(-0.0)
    c["w"] = (0.4 * rng.standard_normal((ny, nz, nx))).astype(f32)
    c["dqdt_w"] = (0.4 * rng.standard_normal((ny, nz, nx))).astype(f32)
    c["adjust"] = bool(pressure)
    return c


def fingerprint(c):
    tot = 0.0
    for g in ("hi", "hi_u", "hi_v"):
        tot += sum(float(c[g][k].astype(np.float64).sum()) for k in ("lon", "lat", "z"))
    for k in ("lo_lon", "lo_lat", "lo_z", "w", "dqdt_w"):
        tot += float(c[k].astype(np.float64).sum())
    for lo in (c["lo1"], c["lo2"]):
        tot += sum(float(lo[n].astype(np.float64).sum()) for n in FORCED)
    return tot


LUT_KEYS = ("x", "y", "w", "z", "zw")


def attach_luts(c, luts):
    """luts: {"geo" / "geo_u" / "geo_v": {x, y, w, z, zw}} as geo_LUT / vLUT made them (a fixture's, or the compiled reference's)"""
    for g, hi in (("geo", "hi"), ("geo_u", "hi_u"), ("geo_v", "hi_v")):
        G = {k: np.ascontiguousarray(luts[g][k], f32 if k in ("w", "zw") else np.int32) for k in LUT_KEYS}      # (a fixture stores small indices as bytes)
        G["i0"], G["j0"] = int(c[hi].get("i0", 0)), int(c[hi].get("j0", 0))
        c[g] = G
    # forcing%geo%z: the forcing's z on the model's columns, geo_interp alone
    c["geo_z"] = geo_novert(c["lo_z"], c["geo"], c["lo_z"].shape[1])
    if not c["adjust"]:
        raise_if = c["lo_z"].shape[1] >= c["z"].shape[1]
        assert not raise_if, "a case without the pressure adjustment is one whose forcing has fewer levels than the model"
    return c


def load_case(name):
    """a stored case: the inputs made again from the recipe (their fingerprint checked), the tables from the fixture"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = make_inputs(**json.loads(str(z["params"])))
    assert abs(fingerprint(c) - float(z["input_fingerprint"])) <= 1e-9 * abs(float(z["input_fingerprint"])), "the case recipe no longer makes the fixture's inputs"
    attach_luts(c, {g: {k: z[f"{g}_{k}"] for k in LUT_KEYS} for g in ("geo", "geo_u", "geo_v")})
    return c, z


def forced_of(c):
    """the forced set of a case: without the pressure where adjust_pressure cannot run"""
    return [n for n in FORCED if n != "pressure" or c["adjust"]]


def random_luts(rng, nx, nz, ny, nxf, nzf, nyf, i0=0, j0=0):
    """valid tables that no geometry made: every corner, level and weight drawn at random (the device and the restatement gather
    through the same ones), levels below / above the grid (equal indices, weights 0.5) in a tenth of the cells each"""
    G = {"x": rng.integers(1, nxf + 1, (ny, nx, 4)).astype(np.int32), "y": rng.integers(1, nyf + 1, (ny, nx, 4)).astype(np.int32)}
    w = rng.random((ny, nx, 4)); w[..., :3] /= w[..., :3].sum(axis=-1, keepdims=True)
    G["w"] = w.astype(f32)
    z1 = rng.integers(1, max(nzf, 2), (ny, nz, nx))
    z = np.stack([z1, np.minimum(z1 + 1, nzf)], axis=-1)
    w1 = rng.random((ny, nz, nx))
    zw = np.stack([w1, 1.0 - w1], axis=-1)
    r = rng.random((ny, nz, nx))
    z[r < 0.1] = 1; z[r > 0.9] = nzf; zw[(r < 0.1) | (r > 0.9)] = 0.5
    G["z"], G["zw"] = z.astype(np.int32), zw.astype(f32)
    G["i0"], G["j0"] = i0, j0
    return G


def random_case(seed, nx, nz, ny, nxf, nzf, nyf, nsmooth=1, ext=(1, 1, 1, 1)):
    """a case on tables that no geometry made (random_luts), for the shapes no fixture has: forcing arrays of two steps, rising z
    columns for adjust_pressure (run only where nzf >= nz), w and its dqdt"""
    rng = np.random.default_rng(4200 + seed)
    w_, e_, s_, n_ = ext
    c = {"nsmooth": int(nsmooth), "adjust": nzf >= nz}
    c["geo"] = random_luts(rng, nx, nz, ny, nxf, nzf, nyf)
    c["geo_u"] = random_luts(rng, nx + 1 + w_ + e_, nz, ny + s_ + n_, nxf, nzf, nyf, w_, s_)
    c["geo_v"] = random_luts(rng, nx + w_ + e_, nz, ny + 1 + s_ + n_, nxf, nzf, nyf, w_, s_)
    c["z"] = np.cumsum(rng.uniform(20.0, 700.0, (ny, nz, nx)), axis=1).astype(f32)
    c["geo_z"] = np.cumsum(rng.uniform(20.0, 700.0, (ny, nzf, nx)), axis=1).astype(f32)
    sf = (nyf, nzf, nxf)

    def forcing_fields():
        out = {"water_vapor": rng.uniform(0.0, 0.012, sf), "potential_temperature": rng.uniform(270.0, 330.0, sf),
               "pressure": rng.uniform(20000.0, 101000.0, sf), "u": 10.0 * rng.standard_normal(sf), "v": 10.0 * rng.standard_normal(sf)}
        return {k: np.ascontiguousarray(v, f32) for k, v in out.items()}
    c["lo1"], c["lo2"] = forcing_fields(), forcing_fields()
    c["w"] = rng.standard_normal((ny, nz, nx)).astype(f32)
    c["dqdt_w"] = rng.standard_normal((ny, nz, nx)).astype(f32)
    return c


# ---- the same on the device -----------------------------------------------------------------------------------------------------------
def boundary_of(c, lo, fields=None):
    from icar_amd.forcing import boundary_t, geo_t
    sf = lambda n: c["lo1"][n].shape
    g = geo_t(*(c["geo"][k] for k in LUT_KEYS), forcing_shape=sf("pressure"), geo_z=c["geo_z"])
    gu = geo_t(*(c["geo_u"][k] for k in LUT_KEYS), forcing_shape=sf("u"), i0=c["geo_u"]["i0"], j0=c["geo_u"]["j0"])
    gv = geo_t(*(c["geo_v"][k] for k in LUT_KEYS), forcing_shape=sf("v"), i0=c["geo_v"]["i0"], j0=c["geo_v"]["j0"])
    return boundary_t(g, gu, gv, {n: lo[n] for n in (fields or forced_of(c))})


def device_domain(c, configure=True):
    """a single-image domain_t of the case's tile with forcing_configure done"""
    from icar_amd.domain import domain_t
    from icar_amd.grid import grid_t
    from icar_amd.forcing import forcing_configure
    ny, nz, nx = c["z"].shape
    d = domain_t(grid_t().set_grid_dimensions(nx, ny, nz, 1, 1), device=0, dx=2000.0)
    if configure:
        forcing_configure(d, boundary_of(c, c["lo1"]), c["nsmooth"], domain_z=c["z"] if c["adjust"] else None)
    return d


def device_two_steps(d, c):
    """the two carried forcing steps on the device, entry point by entry point; returns what run_oracle returns (without the flags)"""
    from icar_amd.forcing import forcing_download
    names = forced_of(c)
    d.interpolate_forcing(boundary_of(c, c["lo1"]), update=False)
    data = {n: d.get(n) for n in names}
    lo = {"u1": forcing_download(d, "u", c["lo1"]["u"].shape), "v1": forcing_download(d, "v", c["lo1"]["v"].shape)}
    d.set("w", c["w"]); data["w"] = c["w"]
    d.interpolate_forcing(boundary_of(c, c["lo2"]), update=True)
    pre = {n: d.get_dqdt(n) for n in names}
    lo.update({"u2": forcing_download(d, "u", c["lo2"]["u"].shape), "v2": forcing_download(d, "v", c["lo2"]["v"].shape)})
    d.set_dqdt("w", c["dqdt_w"])
    d.update_delta_fields(DT_SECONDS)
    dq = {n: d.get_dqdt(n) for n in names + ["w"]}
    return data, pre, dq, lo

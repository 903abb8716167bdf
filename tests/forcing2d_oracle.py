"""TEST INFRASTRUCTURE: loader of tests/support/forcing2d_oracle.c (the CPU restatement of the 2-D forced variables: the product's own
header icar_amd/csrc/forcing2d_cell.h compiled for the host), the chain interpolate / delta / apply assembled from it, and the recipe of
the test cases.  The geometry and the geolut tables are those of tests/forcing_oracle.py:CASES (read-only: the tables come from the
tests/golden/forcing_*.npz fixtures and are held to a checksum stored beside the 2-D results).  The library is compiled with
gcc -O2 -ffp-contract=off on first use and by __graft_entry__.build(), so that it exists where the GPU tests run.

Arrays are numpy in C order == the reference's Fortran order read backwards: data_2d / dqdt_2d (ny, nx), a forcing variable (ny_f, nx_f),
geolut x / y / w (ny, nx, 4).  accumulated_precipitation%data_2dd is REAL(8)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import forcing_oracle as FO  # noqa: E402

SRC = os.path.join(HERE, "support", "forcing2d_oracle.c")
HDR = os.path.join(ROOT, "icar_amd", "csrc", "forcing2d_cell.h")
LIB = os.path.join(HERE, "support", "libforcing2d_oracle.so")
GOLDEN = os.path.join(HERE, "golden")
f32 = np.float32
VARS = ["sst", "shortwave", "longwave", "external_precipitation"]            # enum icar_hip_forced2d, in its order
INTERVAL_DT = [3600.0, 10800.0]                                              # dt%seconds() of the two forcing intervals
APPLY_DT = [[17.3, 20.0, 7.0625], [33.7, 12.5]]                              # the sub-steps behind each; 17.3 and 33.7 are no REAL(4)
CASES = {n: "forcing2d_" + n[len("forcing_"):] for n in FO.CASES}            # 3-D case name -> 2-D fixture name
CONSTANT_CASE, NEGZERO_CASE = "forcing_c_top_24x8x16", "forcing_f_wide_5x6x14"
_lib = None


def build(force=False, contract=False, out=None):
    out = out or LIB
    if force or not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(out):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-DF2_CONTRACT=%d" % int(contract), SRC, "-o", out])
    return out


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bitdiff(a, b):
    """the number of elements whose bit patterns differ (REAL(4) or REAL(8))"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return int((a.view(u) != b.view(u)).sum())


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def geo_interp2d(lo, G, L=None):
    L = L or lib()
    ny, nx, _ = G["x"].shape
    nyf, nxf = lo.shape
    assert lo.dtype == f32 and lo.flags.c_contiguous
    out = np.empty((ny, nx), f32)
    ci = ctypes.c_int
    L.f2o_geo_interp2d(_p(lo), ci(nxf), ci(nyf), _p(G["x"]), _p(G["y"]), _p(G["w"]), ci(nx), ci(ny), _p(out))
    return out


def delta(dqdt, data, dt, L=None):
    """in place on dqdt"""
    assert dqdt.dtype == f32 and data.dtype == f32 and dqdt.flags.c_contiguous and data.flags.c_contiguous and dqdt.shape == data.shape
    (L or lib()).f2o_delta(_p(dqdt), _p(data), ctypes.c_size_t(dqdt.size), ctypes.c_double(dt))


def apply(x, dqdt, dt, L=None):
    """in place on x"""
    assert x.dtype == f32 and dqdt.dtype == f32 and x.flags.c_contiguous and dqdt.flags.c_contiguous and x.shape == dqdt.shape
    (L or lib()).f2o_apply(_p(x), _p(dqdt), ctypes.c_size_t(x.size), ctypes.c_double(dt))


def precip(acc, ext, dt, L=None):
    """in place on the REAL(8) acc"""
    assert acc.dtype == np.float64 and ext.dtype == f32 and acc.flags.c_contiguous and ext.flags.c_contiguous and acc.shape == ext.shape
    (L or lib()).f2o_precip(_p(acc), _p(ext), ctypes.c_size_t(acc.size), ctypes.c_double(dt))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def fields(rng, nyf, nxf, shift, constant=False, negzero=False):
    """one forcing time: SST 270 .. 300 K, fluxes 0 .. 1000 W m-2 with a night side of exact zeros, a precipitation rate [mm / s] that is
    zero in a third of the cells.  FP64, rounded once to REAL(4)."""
    jf, if_ = np.meshgrid(np.arange(nyf, dtype=np.float64), np.arange(nxf, dtype=np.float64), indexing="ij")
    sst = np.clip(285.0 + shift + 12.0 * np.sin(0.7 * if_ + 0.3) * np.cos(0.5 * jf) + rng.normal(0, 1.0, (nyf, nxf)), 270.0, 300.0)
    sun = np.sin(0.9 * if_ - 0.4 * jf + 0.8 * shift)
    sw = np.where(sun > 0.0, np.minimum(1000.0 * sun * rng.uniform(0.6, 1.0, (nyf, nxf)), 1000.0), 0.0)
    n = nyf * nxf
    dark = rng.permutation(n).reshape(nyf, nxf) < (n + 3) // 4       # a quarter of the cells are night whatever the sine says
    sw[dark] = 0.0
    lw = 300.0 + 25.0 * shift + 120.0 * rng.uniform(-1.0, 1.0, (nyf, nxf))
    dry = rng.permutation(n).reshape(nyf, nxf) < (n + 2) // 3        # a third of the cells, exactly
    rate = np.where(dry, 0.0, 2.0e-3 * rng.exponential(1.0, (nyf, nxf)))
    if constant:
        lw = np.full((nyf, nxf), 312.5)
    out = {"sst": sst, "shortwave": sw, "longwave": lw, "external_precipitation": rate}
    out = {k: np.ascontiguousarray(v, f32) for k, v in out.items()}
    if negzero:                                                   # every sum that starts from 0 gives +0
        for k in ("shortwave", "external_precipitation"):
            out[k][out[k] == 0] = f32(-0.0)
    return out


def make_inputs(name, params=None):
    """the 2-D inputs of a case of forcing_oracle.CASES / EXTRA_SEEDS: three forcing times (the initial one and two updates) of the four
    variables on the case's forcing grid, and the accumulated precipitation the run starts from"""
    q = params or {**FO.CASES, **FO.EXTRA_SEEDS}[name]
    rng = np.random.default_rng(7300 + q["seed"])
    lo = [fields(rng, q["nyf"], q["nxf"], s, constant=name == CONSTANT_CASE, negzero=name == NEGZERO_CASE) for s in (0.0, 1.5, -1.0)]
    assert min((l["external_precipitation"] == 0).mean() for l in lo) >= 0.2 and all((l["shortwave"] == 0).any() for l in lo)
    return {"name": name, "nx": q["nx"], "ny": q["ny"], "lo": lo, "acc0": rng.uniform(0.0, 50.0, (q["ny"], q["nx"]))}


def random_case(seed, nx, ny, nxf=2, nyf=2):
    """a case on tables that no geometry made (forcing_oracle.random_luts), for the shapes no fixture has"""
    rng = np.random.default_rng(5100 + seed)
    G = FO.random_luts(rng, nx, 2, ny, nxf, 2, nyf)
    lo = [fields(rng, nyf, nxf, s) for s in (0.0, 1.5, -1.0)]
    return {"name": f"random{seed}", "nx": nx, "ny": ny, "lo": lo, "acc0": rng.uniform(0.0, 50.0, (ny, nx)), "G": G, "luts": G}


def lut_sha(G):
    return FO.sha(np.concatenate([np.ascontiguousarray(G[k]).view(np.uint32).ravel() for k in ("x", "y", "w")]))


def load_case(name):
    """a stored case: the inputs made again from the recipe, the geolut from the 3-D fixture (its checksum held to the 2-D fixture's),
    the reference's results.  Returns (case, fixture, the 3-D case for forcing_oracle.device_domain)"""
    c3, _ = FO.load_case(name)
    z = np.load(os.path.join(GOLDEN, CASES[name] + ".npz"))
    c = make_inputs(name)
    c["G"] = c3["geo"]
    assert lut_sha(c["G"]) == str(z["lut_sha"]), "the geolut of the 3-D fixture is not the one the 2-D results were made with"
    assert abs(fingerprint(c) - float(z["input_fingerprint"])) <= 1e-9 * abs(float(z["input_fingerprint"])), "the case recipe no longer makes the fixture's inputs"
    return c, z, c3


def fingerprint(c):
    return float(c["acc0"].sum()) + sum(float(l[v].astype(np.float64).sum()) for l in c["lo"] for v in VARS)


def run_oracle(c, L=None, enabled=VARS, have_acc=True, no_data=()):
    """the chain of a case: {stage: array}.  init_<v>: interpolate (update = .false.); per interval n: i<n>_pre_<v> interpolate (update),
    i<n>_dq_<v> the delta, i<n>_a<k>_<v> and i<n>_a<k>_acc after the k-th apply.  enabled: the variables apply_forcing handles (all are
    interpolated and get their delta); have_acc = False: no accumulated precipitation; no_data: variables whose data_2d does not exist
    (they are not interpolated with update = .false. and apply_forcing passes them over)"""
    G = c["G"]
    out, data, dq = {}, {}, {}
    for v in VARS:
        if v not in no_data:
            data[v] = geo_interp2d(c["lo"][0][v], G, L)
            out[f"init_{v}"] = data[v].copy()
    acc = c["acc0"].copy()
    for n in (1, 2):
        for v in VARS:
            dq[v] = geo_interp2d(c["lo"][n][v], G, L)
            out[f"i{n}_pre_{v}"] = dq[v].copy()
        for v in VARS:
            if v in data:
                delta(dq[v], data[v], INTERVAL_DT[n - 1], L)
                out[f"i{n}_dq_{v}"] = dq[v].copy()
        for k, dt in enumerate(APPLY_DT[n - 1]):
            for v in VARS:
                if v in enabled and v in data:
                    apply(data[v], dq[v], dt, L)
            if "external_precipitation" in enabled and "external_precipitation" in data and have_acc:
                precip(acc, data["external_precipitation"], dt, L)
            for v in data:
                out[f"i{n}_a{k}_{v}"] = data[v].copy()
            out[f"i{n}_a{k}_acc"] = acc.copy()
    return out


# ---- the same on the device -----------------------------------------------------------------------------------------------------------
def device_domain(c, nz=2):
    """a single-image domain_t of the case's tile with forcing_configure done from c["luts"] (random_case)"""
    from icar_amd.domain import domain_t
    from icar_amd.grid import grid_t
    from icar_amd.forcing import forcing_configure, boundary_t, geo_t
    G = c["luts"]
    d = domain_t(grid_t().set_grid_dimensions(c["nx"], c["ny"], nz, 1, 1), device=0, dx=2000.0)
    nyf, nxf = c["lo"][0]["sst"].shape
    forcing_configure(d, boundary_t(geo_t(*(G[k] for k in FO.LUT_KEYS), forcing_shape=(nyf, 2, nxf))), 1)
    return d


def device_chain(d, c, enabled=VARS, have_acc=True, no_data=(), fused=None):
    """run_oracle's chain on the device, entry point by entry point.  fused: a callable (d, n) that makes interval n's interpolate
    (update) and delta in its own way (the forcing step); the `pre` stages are then absent"""
    from icar_amd import forcing as F
    out = {}
    with_data = [v for v in VARS if v not in no_data]
    for v in VARS:
        F.forcing2d_upload(d, v, c["lo"][0][v])
    d.interpolate_forcing_2d(with_data, update=False)
    for v in with_data:
        out[f"init_{v}"] = F.forcing2d_get(d, v)
    if have_acc:
        d.set("accumulated_precipitation", c["acc0"])
    F.forcing2d_enable(d, list(enabled))
    for n in (1, 2):
        for v in VARS:
            F.forcing2d_upload(d, v, c["lo"][n][v])
        if fused is not None:
            fused(d, n)
        else:
            d.interpolate_forcing_2d(VARS, update=True)
            for v in VARS:
                out[f"i{n}_pre_{v}"] = F.forcing2d_get(d, v, dqdt=True)
            d.update_delta_fields_2d(with_data, INTERVAL_DT[n - 1])
        for v in with_data:
            out[f"i{n}_dq_{v}"] = F.forcing2d_get(d, v, dqdt=True)
        for k, dt in enumerate(APPLY_DT[n - 1]):
            d.apply_forcing_2d(dt)
            for v in with_data:
                out[f"i{n}_a{k}_{v}"] = F.forcing2d_get(d, v)
            out[f"i{n}_a{k}_acc"] = d.get("accumulated_precipitation") if have_acc else c["acc0"].copy()
    return out

"""First measurement of the 2-D forced variables (profiles/r23_steps.md) at 512 x 512 from a 64 x 64 forcing grid with all four variables:
the three kernels by the library's HIP-event timers; icar_hip_forcing_step with the family enabled against the same call without it
(512 x 512 x 40, two scalars and the winds forced); the four uploads; what the family replaces -- four 512 x 512 arrays down and up per
sub-step; and bench.py's step (MPDATA + Thompson, icar_hip_step_n) with the family enabled against the same step without it.
    python profiles/micro/forcing2d_time.py [out.json]
The tables are geometric (neighbouring columns name neighbouring forcing cells), not random: the gather's cache behaviour is a run's."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from forcing_time import tables, read  # noqa: E402
from icar_amd import forcing as F  # noqa: E402
from icar_amd.capi import lib, check  # noqa: E402
from icar_amd.domain import domain_t  # noqa: E402
from icar_amd.grid import grid_t  # noqa: E402
from icar_amd.options import options_t  # noqa: E402

f32 = np.float32
NX, NZ, NY, NXF, NYF = 512, 40, 512, 64, 64
VARS = ["sst", "shortwave", "longwave", "external_precipitation"]
KEYS = ("x", "y", "w", "z", "zw")
GROUPS = ("forcing2d_interp", "forcing2d_delta", "forcing2d_apply")


def wall(fn, d, reps=7):
    """median and minimum of the host's clock around fn() and a synchronise, in microseconds"""
    t = []
    for _ in range(reps):
        d.synchronize()
        t0 = time.perf_counter()
        fn()
        d.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": statistics.median(t), "min_us": min(t)}


def forcing_side():
    rng = np.random.default_rng(2)
    sf, e = (NYF, 30, NXF), 2
    g = tables(rng, NX, NY, NZ, NXF, 30, NYF)
    gu = tables(rng, NX + 1 + 2 * e, NY + 2 * e, NZ, NXF, 30, NYF, e, e)
    gv = tables(rng, NX + 2 * e, NY + 1 + 2 * e, NZ, NXF, 30, NYF, e, e)
    names = ["water_vapor", "potential_temperature", "u", "v"]
    lo = {n: rng.uniform(280.0, 320.0, sf).astype(f32) for n in names}
    b = F.boundary_t(F.geo_t(*(g[k] for k in KEYS), forcing_shape=sf), F.geo_t(*(gu[k] for k in KEYS), forcing_shape=sf, i0=e, j0=e),
                     F.geo_t(*(gv[k] for k in KEYS), forcing_shape=sf, i0=e, j0=e), lo)
    d = domain_t(grid_t().set_grid_dimensions(NX, NY, NZ, 1, 1), device=0, dx=2000.0)
    F.forcing_configure(d, b, 2)
    for k, s in (("jacobian", (NY, NZ, NX)), ("jacobian_u", (NY, NZ, NX + 1)), ("jacobian_v", (NY + 1, NZ, NX)), ("jacobian_w", (NY, NZ, NX)), ("advection_dz", (NY, NZ, NX))):
        d.set(k, rng.uniform(0.9, 1.1, s).astype(f32) * (200.0 if k == "advection_dz" else 1.0))
    d.set("sintheta", np.zeros((NY, NX))); d.set("costheta", np.ones((NY, NX)))
    d.interpolate_forcing(b, update=False)
    d.set("w", np.zeros((NY, NZ, NX), f32))
    lo2 = {v: rng.uniform(0.0, 300.0, (NYF, NXF)).astype(f32) for v in VARS}
    out = {"uploads_of_four_64x64": wall(lambda: [F.forcing2d_upload(d, v, lo2[v]) for v in VARS], d)}
    d.interpolate_forcing_2d(VARS, update=False)
    d.set("accumulated_precipitation", np.zeros((NY, NX)))
    opt = options_t(); opt.physics.windtype = 0
    stepf = lambda: F.forcing_step(d, b, opt, 3600.0, upload=False)
    stepf(); stepf()                                              # the first pays the allocations
    F.forcing2d_enable(d, [])
    off = wall(stepf, d)
    F.forcing2d_enable(d, VARS)
    stepf()
    on = wall(stepf, d)
    F.forcing2d_enable(d, [])
    off2 = wall(stepf, d)
    out["forcing_step_disabled"], out["forcing_step_enabled"], out["forcing_step_disabled_again"] = off, on, off2
    # the kernels, by the event timers, 20 calls each
    F.forcing2d_enable(d, VARS)
    check(lib().icar_hip_timing_reset(d.ctx), "timing_reset"); check(lib().icar_hip_timing_enable(d.ctx, 1), "timing_enable")
    for _ in range(20):
        d.interpolate_forcing_2d(VARS, update=True)
        d.update_delta_fields_2d(VARS, 3600.0)
        d.apply_forcing_2d(17.3)
    d.synchronize()
    check(lib().icar_hip_timing_enable(d.ctx, 0), "timing_enable")
    n2 = NX * NY
    # compulsory bytes: interp 48 B of tables per cell and variable (each block reads its own) + 4 written; delta 4 + 4 read, 4 written;
    # apply (4 + 4 read, 4 written) x 4 variables + 4 (the rate again) + 8 + 8 for the REAL(8) sum
    nbytes = {"forcing2d_interp": n2 * 4 * 52, "forcing2d_delta": n2 * 4 * 12, "forcing2d_apply": n2 * (4 * 12 + 20)}
    for grp in GROUPS:
        ms, n = read(d, grp)
        us = ms * 1e3 / max(n, 1)
        out[grp] = {"us_per_launch": us, "launches": n, "bytes": nbytes[grp], "TBps": nbytes[grp] / (us * 1e-6) / 1e12 if us else None}
    # what the family replaces: the four arrays down and up, per sub-step
    host = {}

    def down():
        for v in VARS: host[v] = F.forcing2d_get(d, v)

    def up():
        for v in VARS: F.forcing2d_set(d, v, host[v])
    out["four_512x512_down"] = wall(down, d)
    out["four_512x512_up"] = wall(up, d)
    d.close()
    return out


def step_side(steps=20, rounds=3):
    import bench
    args = argparse.Namespace(nx=NX, ny=NY, nz=NZ, hill=1000.0, adv="mpdata", mp="thompson", scaling="strong")
    d, opt, case, g = bench.build_tile(args, 0, 1, 0)
    rng = np.random.default_rng(3)
    G = tables(rng, NX, NY, NZ, NXF, 2, NYF)
    F.forcing_configure(d, F.boundary_t(F.geo_t(*(G[k] for k in KEYS), forcing_shape=(NYF, 2, NXF))), 1)
    for s in (0.0, 1.0):
        for v in VARS:
            F.forcing2d_upload(d, v, (rng.uniform(0.0, 300.0, (NYF, NXF)) * (1e-5 if v == "external_precipitation" else 1.0)).astype(f32))
        d.interpolate_forcing_2d(VARS, update=bool(s))
    d.update_delta_fields_2d(VARS, 3600.0)
    bench.run_steps(d, opt, 5); d.synchronize()
    res = {"disabled": [], "enabled": []}
    for _ in range(rounds):
        for which in ("disabled", "enabled"):
            F.forcing2d_enable(d, VARS if which == "enabled" else [])
            d.synchronize()
            t0 = time.perf_counter()
            bench.run_steps(d, opt, steps)
            d.synchronize()
            res[which].append((time.perf_counter() - t0) * 1e3 / steps)
    d.close()
    return {"steps_per_window": steps, "ms_per_step": res, "median_disabled": statistics.median(res["disabled"]),
            "median_enabled": statistics.median(res["enabled"])}


if __name__ == "__main__":
    res = {"tile": [NX, NY], "forcing_grid": [NXF, NYF], "forcing_side": forcing_side(), "step_side": step_side()}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)

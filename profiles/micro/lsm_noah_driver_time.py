#!/usr/bin/env python
"""Times of the Noah branch of lsm() on the MI355X: the kernels around k_noah beside k_noah itself, in the same run.

    python profiles/micro/lsm_noah_driver_time.py [--calls 20] [--out FILE.json]     512 x 512

State: the surface of tests/lsm_noah_driver_oracle.py (a Noah case of tests/noah_oracle.py with the 10 m winds, the terrain and the
accumulated precipitation around it) after lsm_init, the coupling and one call.  Every timed call is icar_hip_lsm with the gate open (the
clock is moved by update_interval in front of it, outside the timers): the event timers "lsm_noah_pre", "lsm_noah" and "lsm_noah_post" around
the three launches, "lsm_fluxes" around apply_fluxes, and the host's wall clock around the whole call with a synchronize behind it.
Bytes the two kernels must move per cell: pre reads 9 REAL(4), the land mask and two REAL(8) and writes 6 REAL(4) = 80 B; post reads 14
REAL(4) (four of them soil layers) and one REAL(8) and writes 7 REAL(4) and one REAL(8) = 100 B.

Also timed, the way round 20 timed its transfers (the host's wall clock around the copies, synchronized): what a host no longer moves per
update -- CHS, Ri, QGH and current_precipitation up; temperature, water_vapor (a level each), surface_pressure, skin_temperature, u_10m,
v_10m and the accumulated precipitation down."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(512, 512)]
BYTES = {"lsm_noah_pre": 80, "lsm_noah_post": 100, "lsm_noah": 460}
GROUPS = ["lsm_noah_pre", "lsm_noah", "lsm_noah_post", "lsm_fluxes"]


def timed(args):
    import lsm_noah_driver_oracle as LN
    import noah_oracle as N
    from icar_amd import surface
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    tab = N.load_tables()
    for nx, ny in SIZES:
        q = dict(nx=nx, ny=ny, seed=1234, dt=1200.0, t=[270.0, 273.0], sw=[100, 600], pr=[[0.5, 3.0], [0.5, 3.0]], snow0=0.4, soil_t=272.5)
        c = LN.make_case(tab, noah=q, seed=1234, closed=99, max_swe=1e10)
        d = LN.device_domain(tab, c)
        LN.device_call(d, c, 0)
        LN.device_forcing(d, c, 1)
        now = c["clock"][0]

        def call():
            nonlocal now
            now += float(c["update_interval"])
            d.model_time_seconds = now
            d.synchronize()
            t0 = time.perf_counter()
            surface.lsm(d, d._lnd_opt, 30.0)
            d.synchronize()
            return time.perf_counter() - t0
        for _ in range(3):
            call()
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, ",".join(GROUPS).encode()), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        wall = [call() for _ in range(args.calls)]
        d.synchronize()
        cells = nx * ny
        res = {"calls": args.calls, "icar_hip_lsm_wall_us": {"median": float(np.median(wall)) * 1e6, "min": float(min(wall)) * 1e6}}
        for g in GROUPS:
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, g.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            us = ms.value / args.calls * 1e3
            res[g] = {"scopes": n.value, "us_per_call": us, "ns_per_cell": us * 1e3 / cells}
            if g in BYTES and us > 0:
                res[g]["GBps"] = BYTES[g] * cells / (us * 1e-6) / 1e9
        check(L.icar_hip_timing_enable(d.ctx, 0), "timing_enable")
        # the transfers a host no longer makes per update
        up = {k: np.ascontiguousarray(LN.device_get(d, k)) for k in ("chs", "rib", "qgh", "rainbl_step")}
        moves = []
        for _ in range(5):
            d.synchronize()
            t0 = time.perf_counter()
            for k, a in up.items():
                surface.noah_set(d, LN.NOAH_OF[k], a)
            t1 = time.perf_counter()
            for k in ("temperature", "water_vapor", "surface_pressure", "skin_temperature", "u_10m", "v_10m", "accumulated_precipitation"):
                d.get(k)
            d.synchronize()
            moves.append((t1 - t0, time.perf_counter() - t1))
        res["transfers_saved_per_update_us"] = {"up_4_arrays": float(np.median([m[0] for m in moves])) * 1e6,
                                                "down_7_fields_two_levels_each_3d": float(np.median([m[1] for m in moves])) * 1e6}
        out[f"{nx}x{ny}"] = res
        d.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = timed(a)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

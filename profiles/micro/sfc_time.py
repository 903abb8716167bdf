#!/usr/bin/env python
"""Times of the three surface-flux kernels (k_diag_10m, k_water_simple, k_apply_fluxes) alone on the MI355X.

    python profiles/micro/sfc_time.py [--calls 200] [--out FILE.json]     the event timers "diag_10m", "lsm_water", "lsm_fluxes" at 512x512x40

State: the recipe of the tests (tests/sfc_oracle.py: half the cells open water, every branch taken).  water_simple rewrites
roughness_z0 from ustar, which the calls here do not change, so the calls are not reset between; apply_fluxes adds the same
increment every call (a few 1e-3 K), the floor is reached in the first.  Bytes k_apply_fluxes must move: 4 B per cell of qv read
(every level of every column: the floor) + 24 B per cell of the tile's nz + 1 surface levels (theta and qv read and written, density,
exner, dz read; the floor's writes elsewhere happen once) -- at 40 levels and a 6-level layer 4 + 24 x 7 / 40 = 8.2 B/cell.  Rates
are compared with the 6.3 TB/s the microarchitecture guide gives as achievable HBM bandwidth and with the streaming rows of DESIGN."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(512, 512, 40)]
HBM = 6.3e12


def timed(args):
    import sfc_oracle as S
    from icar_amd import surface
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    for nx, ny, nz in SIZES:
        c = S.make_case(nx, ny, nz, seed=1234)
        d = S.device_domain(c)
        layers = S.layers(c)
        calls = {"diag_10m": lambda: surface.diag_10m(d), "lsm_water": lambda: surface.water_simple(d),
                 "lsm_fluxes": lambda: surface.apply_fluxes(d, 60.0, 2, nx - 1, 2, ny - 1, 1, nz)}
        cells, cols = nx * ny * nz, nx * ny
        byts = {"diag_10m": 32.0 * cols, "lsm_water": 0.5 * 68.0 * cols + 4.0 * cols, "lsm_fluxes": 4.0 * cells + 24.0 * (layers + 1) * (nx - 2) * (ny - 2)}
        for group, call in calls.items():
            for _ in range(10):
                call()
            check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, group.encode()), "timing_groups")
            check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
            for _ in range(args.calls):
                call()
            d.synchronize()
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, group.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            check(L.icar_hip_timing_enable(d.ctx, 0), "timing_enable")
            per = ms.value / n.value
            out[f"{group}/{nx}x{ny}x{nz}"] = {"calls": n.value, "us_per_call": per * 1e3, "bytes": byts[group], "GBps": byts[group] / (per * 1e-3) / 1e9,
                                              "share_of_6.3TBps": byts[group] / (per * 1e-3) / HBM, "surface_levels": layers + 1}
            print(f"{group}/{nx}x{ny}x{nz}", json.dumps(out[f"{group}/{nx}x{ny}x{nz}"]), flush=True)
        d.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", metavar="FILE.json", help="also merge the result into this JSON file")
    args = ap.parse_args()
    res = {"sfc": timed(args)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)

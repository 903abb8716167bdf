#!/usr/bin/env python
"""Times of the YSU boundary-layer slot's kernels alone on the MI355X.

    python profiles/micro/ysu_time.py [--calls 20] [--out FILE.json]     the event timers "ysu_sfc", "ysu" and "ysu_apply" at 512x512x40

State: the probe state of the tests (tests/ysu_oracle.py: mixed layers of 150 m .. 2.5 km under an inversion over 55 % of the rows, a
surface inversion and a cold skin over the rest, cloud slabs, 30 % water).  Every timed call starts from the same state (the four
scalars are uploaded again in front of it, outside the timers).  "ysu_sfc" is k_ysu_sfc, "ysu" one scope around the launches of
k_ysu_column (one per chunk of 2^17 columns), "ysu_apply" is k_ysu_apply.  The slot as a whole: the sum of the three, and the wall
time of back-to-back icar_hip_pbl calls between two synchronisations.
Bytes the slot must move per cell and call (REAL(4)): k_ysu_column reads ten 3-D inputs and writes six tendencies and exch_h (68 B;
its workspace traffic comes on top and is not compulsory), k_ysu_apply reads four fields and six tendencies and writes the four fields
and the non-zero tendencies back (up to 80 B); the 2-D arrays are 1 / nz of that."""
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
SIZES = [(512, 512, 40)]
GROUPS = ("ysu_sfc", "ysu", "ysu_apply")
BYTES_PER_CELL = {"ysu": 68.0, "ysu_apply": 80.0}


def timed(args):
    import ysu_oracle as Y
    from icar_amd import pbl
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    for nx, ny, nz in SIZES:
        c = Y.make_case(nx=nx, ny=ny, nz=nz, seed=1234, lid=12000.0, regime3=0.0)
        d = Y.device_domain(c)

        def call():
            for k in Y.STATE3:
                d.set(Y.DEVICE_NAME.get(k, k), c[k])
            pbl.pbl(d, d._ysu_opt, 40.0)
        for _ in range(2):
            call()
        kpbl, ri = Y.owned(c, pbl.ysu_get(d, "kpbl")), Y.owned(c, pbl.ysu_get(d, "ri"))
        shares = {"unstable": float((ri <= 0).mean()), "kpbl_is_1": float((kpbl == 1).mean()), "kpbl_mean": float(kpbl.mean()), "kpbl_max": int(kpbl.max())}
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, ",".join(GROUPS).encode()), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(args.calls):
            call()
        d.synchronize()
        key = f"{nx}x{ny}x{nz}"
        cells = nx * ny * nz
        out[key] = {"calls": args.calls, "columns": shares}
        total = 0.0
        for group in GROUPS:
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, group.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            us = ms.value / args.calls * 1e3
            total += us
            out[key][group] = {"scopes": n.value, "us_per_call": us}
            if group in BYTES_PER_CELL:
                out[key][group]["bytes_per_call"] = BYTES_PER_CELL[group] * cells
                out[key][group]["GBps"] = BYTES_PER_CELL[group] * cells / (us * 1e-6) / 1e9
        check(L.icar_hip_timing_enable(d.ctx, 0), "timing_enable")
        d.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            pbl.pbl(d, d._ysu_opt, 40.0)
        d.synchronize()
        wall = (time.perf_counter() - t0) / args.calls * 1e6
        must = sum(BYTES_PER_CELL.values()) * cells
        out[key]["slot"] = {"us_per_call_sum_of_timers": total, "us_per_call_wall_back_to_back": wall, "bytes_per_call": must,
                            "GBps_at_the_sum": must / (total * 1e-6) / 1e9}
        print(key, json.dumps(out[key]), flush=True)
        d.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", metavar="FILE.json", help="also merge the result into this JSON file")
    args = ap.parse_args()
    res = {"ysu": timed(args)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)

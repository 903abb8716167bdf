#!/usr/bin/env python
"""Times of the convection slot's kernels alone on the MI355X.

    python profiles/micro/cu_time.py [--calls 20] [--out FILE.json]     the event timers "cu_bmj" and "cu_stream" at 512x512x40

State: the probe sounding of the tests (tests/bmj_oracle.py: surface temperature 284 .. 306 K along i, relative humidity 0.25 .. 0.97
along j, a capping warm layer over every third column).  Every call starts from the same state (water vapour, potential temperature
and CLDEFI are uploaded again in front of it, outside the timers), so that the share of convecting columns is that of the first
call.  "cu_bmj" is one scope around the four launches (k_cu_load, k_cu_search, k_cu_bmj, k_cu_store) of every chunk of rows of a
call; "cu_stream" is k_cu_zero and k_cu_apply, two scopes per call.  Bytes the streaming pair must move: k_cu_zero writes two
tendencies (8 B per cell), k_cu_apply reads and writes theta and qv, reads two tendencies and reads qc and qi (32 B per cell)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(512, 512, 40)]


def timed(args):
    import bmj_oracle as B
    from icar_amd import convection
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    for nx, ny, nz in SIZES:
        c = B.make_case(nx=nx, ny=ny, nz=nz, seed=1234)
        d = B.device_domain(c)
        cld = np.full((ny, nx), c["cldefi0"], np.float32)

        def call():
            d.set("water_vapor", c["water_vapor"]); d.set("potential_temperature", c["potential_temperature"])
            convection.cu_set(d, "cldefi", cld)
            convection.convect(d, d._cu_opt, 40.0)
        for _ in range(2):
            call()
        rain = B.owned(c, convection.cu_get(d, "raincv"))
        tend = (B.owned(c, convection.cu_get(d, "tend_th")) != 0).any(axis=1) | (B.owned(c, convection.cu_get(d, "tend_qv")) != 0).any(axis=1)
        shares = {"deep": float((rain > 0).mean()), "shallow": float((tend & ~(rain > 0)).mean()), "quiet": float((~tend & ~(rain > 0)).mean())}
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, b"cu_bmj,cu_stream"), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(args.calls):
            call()
        d.synchronize()
        key = f"{nx}x{ny}x{nz}"
        out[key] = {"calls": args.calls, "columns": shares}
        for group in ("cu_bmj", "cu_stream"):
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, group.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            out[key][group] = {"scopes": n.value, "us_per_call": ms.value / args.calls * 1e3}
        cells = nx * ny * nz
        out[key]["cu_stream"]["bytes_per_call"] = 40.0 * cells
        out[key]["cu_stream"]["GBps"] = 40.0 * cells / (out[key]["cu_stream"]["us_per_call"] * 1e-6) / 1e9
        check(L.icar_hip_timing_enable(d.ctx, 0), "timing_enable")
        print(key, json.dumps(out[key]), flush=True)
        d.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", metavar="FILE.json", help="also merge the result into this JSON file")
    args = ap.parse_args()
    res = {"cu": timed(args)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)

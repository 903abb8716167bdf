#!/usr/bin/env python
"""Times of the NSAS scheme's kernels alone on the MI355X.

    python profiles/micro/nsas_time.py [--calls 20] [--out FILE.json]     the event timers "cu_nsas" and "cu_stream" at 512x512x40

State: the sounding of the tests (tests/nsas_oracle.py: surface temperature 284 .. 306 K along i, a boundary layer up to 97 % humid
along j, a moist layer aloft over 55 % of the columns with ascent in it, sheared winds, surface fluxes negative over a fifth of the
columns).  Every call starts from the same state (the four fields the tendencies are applied to are uploaded again in front of it,
outside the timers), so that the share of convecting columns is that of the first call.  "cu_nsas" is one scope around the launches
(k_nsas_limits once, then k_nsas_deep, k_nsas_shallow, k_nsas_finish per chunk of rows); "cu_stream" is k_cu_zero and k_cu_apply, two
scopes per call.  Bytes the streaming pair must move: k_cu_zero writes four tendencies (16 B per cell), k_cu_apply reads and writes
four fields and reads four tendencies (48 B per cell)."""
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
    import nsas_oracle as N
    from icar_amd import convection
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    for nx, ny, nz in SIZES:
        c = N.make_case(nx=nx, ny=ny, nz=nz, seed=1234, dx=4000.0)
        d = N.device_domain(c)
        A = N.state(c)

        def call():
            N.device_put(d, A)
            convection.convect(d, d._cu_opt, 40.0)
        for _ in range(2):
            call()
        # which scheme worked on a column is not among the results (icps is internal; the shallow scheme can rain too): the shares come
        # from the CPU restatement's flags on the same state, whose results the device equals bit for bit
        H = N.state(c)
        N.cu_nsas(c, H, 40.0)
        flags = N.owned(c, H["diag"])
        assert N.bitdiff(N.owned(c, convection.nsas_get(d, "htop")), N.owned(c, H["htop"])) == 0
        deep, shallow = flags & N.D_DEEP_RAIN != 0, flags & N.D_SHALLOW != 0
        shares = {"deep_with_rain": float(deep.mean()), "shallow": float(shallow.mean()), "quiet": float((~deep & ~shallow).mean())}
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, b"cu_nsas,cu_stream"), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(args.calls):
            call()
        d.synchronize()
        key = f"{nx}x{ny}x{nz}"
        out[key] = {"calls": args.calls, "columns": shares}
        for group in ("cu_nsas", "cu_stream"):
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, group.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            out[key][group] = {"scopes": n.value, "us_per_call": ms.value / args.calls * 1e3}
        cells = nx * ny * nz
        out[key]["cu_stream"]["bytes_per_call"] = 64.0 * cells
        out[key]["cu_stream"]["GBps"] = 64.0 * cells / (out[key]["cu_stream"]["us_per_call"] * 1e-6) / 1e9
        out[key]["workspace_MiB"] = (36 * (nz - 1 + 2) + 5) * min(nx * ny, 32768) * 4 / 2 ** 20
        check(L.icar_hip_timing_enable(d.ctx, 0), "timing_enable")
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
            f.write("\n")

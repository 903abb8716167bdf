#!/usr/bin/env python
"""Time of the Noah launch alone on the MI355X.

    python profiles/micro/noah_time.py [--calls 20] [--out FILE.json]     the event timer "lsm_noah" at 512x512

State: the surface of the tests (tests/noah_oracle.py: about an eighth of the cells water, a twentieth land ice, the rest land with every
vegetation and soil category, snow on 40 % of the land) after lsm_init and one call on the host; the timed call is the second one (273 K,
600 W m-2, precipitation on half the cells).  Every call starts from the same state (uploaded again in front of it, outside the timer), so
that the shares of the branches are those of that call; they come from the CPU restatement's flags on the same state, whose results the
device equals bit for bit (asserted here on three arrays).
Bytes the launch must move per cell: it reads 4 words of the atmosphere, the land mask, two categories, 12 read-only and 32 + 16 read-write
words and writes the 48 back: 115 words = 460 B."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(512, 512)]
BYTES_PER_CELL = 4 * (4 + 1 + 2 + 12 + 48 + 48)


def timed(args):
    import noah_oracle as N
    from icar_amd import surface
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    tab = N.load_tables()
    for nx, ny in SIZES:
        c = N.make_case(tab, nx=nx, ny=ny, seed=1234, dt=1200.0, t=[270.0, 273.0], sw=[100, 600], pr=[[0.5, 3.0], [0.5, 3.0]], snow0=0.4, soil_t=272.5)
        A = N.state0(c)
        N.lsm_init(tab, c, A)
        N.lsm_noah(tab, c, A, 0)
        H = {k: v.copy() for k, v in A.items()}
        N.lsm_noah(tab, c, H, 1)
        d = N.device_domain(tab, c)
        N.device_forcing(d, c, 1)

        def call():
            N.device_put(d, A)
            surface.lsm_noah(d, float(c["dt"]), *N.tile_of(c))
        for _ in range(2):
            call()
        for k in ("tsk", "smois", "snow"):
            assert N.bitdiff(N.device_get(d, k), H[k]) == 0, k
        f = H["diag"]
        share = lambda name: float((f & N.D[name] != 0).mean())
        shares = {k.lower(): share(k) for k in ("WATER", "LANDICE", "SFLX", "NOPAC", "SNOPAC_MELT", "SNOPAC_NOMELT", "SMFLX_TWO", "CANRES", "FRH2O_ITER")}
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, b"lsm_noah"), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(args.calls):
            call()
        d.synchronize()
        ms, n = ctypes.c_double(), ctypes.c_int()
        check(L.icar_hip_timing_read(d.ctx, b"lsm_noah", ctypes.byref(ms), ctypes.byref(n)), "timing_read")
        us = ms.value / args.calls * 1e3
        cells = nx * ny
        out[f"{nx}x{ny}"] = {"calls": args.calls, "cells": shares, "lsm_noah": {"scopes": n.value, "us_per_call": us, "ns_per_cell": us * 1e3 / cells,
                                                                           "bytes_per_call": BYTES_PER_CELL * cells,
                                                                           "GBps": BYTES_PER_CELL * cells / (us * 1e-6) / 1e9}}
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

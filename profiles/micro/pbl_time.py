#!/usr/bin/env python
"""Time of the boundary-layer scheme (icar_hip_pbl_simple: k_pbl_coef + k_pbl_diffuse) on the MI355X.

    python profiles/micro/pbl_time.py [--calls 200] [--out FILE.json]     the "pbl" event timers
    python profiles/micro/pbl_time.py --trace                                            20 calls per size without timers, for
        rocprofv3 --kernel-trace --stats -d DIR -o pbl -- python profiles/micro/pbl_time.py --trace
    python profiles/micro/pbl_time.py --parse-stats DIR                                  the two kernels' rows of that run
    python profiles/micro/pbl_time.py --step-cost [--steps 10]                           icar_hip_step_n with the scheme off / on

State: the benchmark's ideal case (bench.py: hill 1000 m, 1 % noise, vapour x 1.4) with the rough-wind recipe of the tests
(tests/pbl_oracle.py: row-wise patchy shear up to 10 m/s, +-0.5 K on theta, 20 % water), dt = 120 s.  Every timed call sees the SAME
state (the six scalars are uploaded again before it, outside the timed group), so the rows' sub-step counts -- printed as a
histogram -- are those of the first call.  Bytes: the scheme must read 12 fields and write 6 (72 B per cell); the two-pass form
moves 48 + 4 B in the coefficient pass and 36 + 24 B in the diffusion pass (112 B per cell).  Rates are compared with the
6.3 TB/s the microarchitecture guide gives as achievable HBM bandwidth."""
import argparse
import csv
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(512, 512, 40), (258, 130, 40)]
HBM = 6.3e12


def make(nx, ny, nz):
    import pbl_oracle as P
    c = P.make_case(nx, ny, nz, seed=1234, rough=10.0, dt=120.0, hill=1000.0)
    c["water_vapor"] = (c["water_vapor"] * np.float32(1.4)).astype(np.float32)
    return P, c


def timed(args):
    from icar_amd import pbl
    from icar_amd.capi import lib, check
    out = {}
    for nx, ny, nz in SIZES:
        P, c = make(nx, ny, nz)
        d = P.device_domain(c)
        L = lib()

        def call():
            for k in P.SCALARS:
                d.set(P.MEMBER[k], c[k])
            pbl.simple_pbl(d, 120.0, 2, nx - 1, 2, ny - 1, 1, nz)

        for _ in range(10):
            call()
        nsub = pbl.nsubsteps(d)[1:-1]
        if not args.trace:
            check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, b"pbl"), "timing_groups")
            check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(20 if args.trace else args.calls):
            call()
        d.synchronize()
        if not args.trace:
            ms, n = ctypes.c_double(), ctypes.c_int()
            check(L.icar_hip_timing_read(d.ctx, b"pbl", ctypes.byref(ms), ctypes.byref(n)), "timing_read")
            per = ms.value / n.value
            cells = (nx - 2) * (ny - 2) * nz
            hist = {int(v): int((nsub == v).sum()) for v in np.unique(nsub)}
            out[f"{nx}x{ny}x{nz}"] = {"calls": n.value, "ms_per_call": per, "cells": cells, "nsubsteps_rows": hist,
                                      "mean_nsubsteps": float(nsub.mean()),
                                      "TBps_at_72B": 72.0 * cells / (per * 1e-3) / 1e12, "TBps_at_112B": 112.0 * cells / (per * 1e-3) / 1e12,
                                      "share_of_6.3TBps_at_72B": 72.0 * cells / (per * 1e-3) / HBM, "share_of_6.3TBps_at_112B": 112.0 * cells / (per * 1e-3) / HBM}
            print(f"{nx}x{ny}x{nz}", json.dumps(out[f"{nx}x{ny}x{nz}"]), flush=True)
        d.close()
    return out


def parse_stats(path):
    rows = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_pbl" in r.get("Name", ""):
                rows[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"]), "avg_ns": float(r["AverageNs"]), "percent": float(r["Percentage"])}
    tot = sum(r["total_ns"] for r in rows.values()) or 1
    for r in rows.values():
        r["share_of_pbl"] = r["total_ns"] / tot
    return rows


def step_cost(args):
    """icar_hip_step_n at 512 x 512 x 40 (the benchmark's configuration: MPDATA + Thompson, its forcing list) with the scheme off and
    on: 6 + 6 alternating runs of --steps steps, each from the initial state, host clock around a device synchronise"""
    from icar_amd import pbl
    from icar_amd.options import options_t
    from icar_amd.microphysics import mp_var_request, mp_init
    from icar_amd.advection import adv_var_request, adv_init
    from icar_amd.time_step import step_n
    from icar_amd.capi import lib, check
    from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kPBL_SIMPLE
    nx, ny, nz = SIZES[0]
    P, c = make(nx, ny, nz)
    forced = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
    restored = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
    runs = {}
    doms = {}
    for name, bl in (("off", 0), ("on", kPBL_SIMPLE)):
        opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON; opt.physics.boundarylayer = bl
        opt.parameters.ideal = True; opt.parameters.dx = float(c["dx"]); opt.parameters.dz_levels = c["dz_levels"]
        mp_var_request(opt); adv_var_request(opt)
        d = P.device_domain(c)
        mp_init(opt, d); adv_init(d, opt); pbl.pbl_init(d, opt)
        for n, _ in forced:
            d.set_dqdt(n, np.zeros(d.shape(d.fid(n)), np.float32))
        d.set("dzdx", np.zeros(d.shape(d.fid("dzdx")), np.float32)); d.set("dzdy", np.zeros(d.shape(d.fid("dzdy")), np.float32))
        doms[name] = (d, opt); runs[name] = []
    for rep in range(7):                                        # the first pair is the warm-up
        for name, (d, opt) in doms.items():
            d.load_case({k: c[k] for k in restored}); d.model_time_seconds = 0.0
            check(lib().icar_hip_mp_reset(d.ctx), "mp_reset")
            d.synchronize()
            t0 = time.perf_counter()
            step_n(d, args.steps, opt, forced=forced)
            d.synchronize()
            if rep: runs[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out = {k: {"ms_per_step": v, "min": min(v), "max": max(v), "median": float(np.median(v))} for k, v in runs.items()}
    out["steps_per_run"] = args.steps
    print("step_cost", json.dumps(out), flush=True)
    for d, _ in doms.values():
        d.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--step-cost", action="store_true")
    ap.add_argument("--parse-stats", metavar="DIR")
    ap.add_argument("--out", metavar="FILE.json", help="also merge the result into this JSON file")
    args = ap.parse_args()
    if args.parse_stats:
        res = {"kernel_trace": parse_stats(args.parse_stats)}
    elif args.step_cost:
        res = {"step_cost": step_cost(args)}
    else:
        res = {"pbl": timed(args)}
    if not args.trace:
        print(json.dumps(res))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            old = json.load(open(args.out)) if os.path.exists(args.out) else {}
            old.update(res)
            json.dump(old, open(args.out, "w"), indent=1)

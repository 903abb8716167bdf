#!/usr/bin/env python
"""Time of the radiation scheme (icar_hip_ra_simple: k_ra_simple) on the MI355X.

    python profiles/micro/ra_time.py [--calls 200] [--out FILE.json]     the "rad" event timers at 512x512x40 and 258x130x40
    python profiles/micro/ra_time.py --step-cost [--steps 10]            icar_hip_step_n with the scheme off / on, 6 + 6 alternating

State: the recipe of the tests (tests/ra_oracle.py: the ideal case with saturated, warm, cloudy and clear columns, latitudes -90 ..
90, longitudes -180 .. 360).  The cooling of one call changes theta by ~1e-3 K, so the calls are not reset between.  Bytes: the
scheme must read theta, pii, qc, qs, qi, qg, qr and write theta on every level (32 B per cell) plus qv, p (and theta, pii again)
on the lowest five levels and ~24 B per column of 2-D traffic: 32 B/cell + (5 x 16 + 24) B/column.  Rates are compared with the
6.3 TB/s the microarchitecture guide gives as achievable HBM bandwidth."""
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
SIZES = [(512, 512, 40), (258, 130, 40)]
HBM = 6.3e12


def timed(args):
    import ra_oracle as R
    from icar_amd import radiation
    from icar_amd.capi import lib, check
    out = {}
    L = lib()
    for nx, ny, nz in SIZES:
        c = R.make_case(nx, ny, nz, seed=1234, D0=100.4)
        d = R.device_domain(c)
        d.model_time_seconds = R.seconds(c, 0)
        call = lambda: radiation.ra_simple(d, 120.0, 2, nx - 1, 2, ny - 1, 1, nz)
        for _ in range(10):
            call()
        check(L.icar_hip_timing_enable(d.ctx, 1), "timing_enable"); check(L.icar_hip_timing_groups(d.ctx, b"rad"), "timing_groups")
        check(L.icar_hip_timing_reset(d.ctx), "timing_reset")
        for _ in range(args.calls):
            call()
        d.synchronize()
        ms, n = ctypes.c_double(), ctypes.c_int()
        check(L.icar_hip_timing_read(d.ctx, b"rad", ctypes.byref(ms), ctypes.byref(n)), "timing_read")
        per = ms.value / n.value
        cells, cols = (nx - 2) * (ny - 2) * nz, (nx - 2) * (ny - 2)
        byts = 32.0 * cells + (5 * 16 + 24) * cols
        out[f"{nx}x{ny}x{nz}"] = {"calls": n.value, "ms_per_call": per, "cells": cells, "bytes": byts, "GBps": byts / (per * 1e-3) / 1e9,
                                  "GBps_at_32B_per_cell": 32.0 * cells / (per * 1e-3) / 1e9, "share_of_6.3TBps": byts / (per * 1e-3) / HBM}
        print(f"{nx}x{ny}x{nz}", json.dumps(out[f"{nx}x{ny}x{nz}"]), flush=True)
        d.close()
    return out


def step_cost(args):
    """icar_hip_step_n at 512 x 512 x 40 (the benchmark's configuration: MPDATA + Thompson, its forcing list) with the scheme off and
    on: 6 + 6 alternating runs of --steps steps, each from the initial state, host clock around a device synchronise"""
    import ra_oracle as R
    from icar_amd import ideal, radiation
    from icar_amd.options import options_t
    from icar_amd.microphysics import mp_var_request, mp_init
    from icar_amd.advection import adv_var_request, adv_init
    from icar_amd.time_step import step_n
    from icar_amd.capi import lib, check
    from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kRA_SIMPLE
    from util import single_image_domain
    nx, ny, nz = SIZES[0]
    c = ideal.make_case(nx, ny, nz, hill_height=1000.0, noise=0.01)
    c["water_vapor"] = (c["water_vapor"] * np.float32(1.4)).astype(np.float32)
    c["latitude"] = (np.linspace(-90.0, 90.0, ny)[:, None] + np.zeros((1, nx))).astype(np.float32)
    c["longitude"] = (np.linspace(-180.0, 360.0, nx)[None, :] + np.zeros((ny, 1))).astype(np.float32)
    forced = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
    restored = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
    runs, doms = {}, {}
    for name, ra in (("off", 0), ("on", kRA_SIMPLE)):
        opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON; opt.physics.radiation = ra
        opt.parameters.ideal = True; opt.parameters.dx = float(c["dx"]); opt.parameters.dz_levels = c["dz_levels"]
        mp_var_request(opt); adv_var_request(opt); radiation.ra_var_request(opt)
        d = single_image_domain(c)
        mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt, date=(2001, 4, 11, 9, 0, 0))
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
    ap.add_argument("--step-cost", action="store_true")
    ap.add_argument("--out", metavar="FILE.json", help="also merge the result into this JSON file")
    args = ap.parse_args()
    res = {"step_cost": step_cost(args)} if args.step_cost else {"rad": timed(args)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)

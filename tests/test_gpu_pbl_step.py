"""The boundary-layer slot of the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:494):
* icar_hip_substep with the scheme configured == the plain sequence diagnostic_update -> pbl -> mp_and_halo -> advect ->
  apply_forcing issued call by call, bit for bit (Thompson and mp_simple);
* icar_hip_step over six or more sub-steps with forced winds and icar_hip_mpdata_exact == the same loop assembled on the CPU from
  the oracle's operators and the PBL restatement, every prognostic field bit for bit;
* with boundarylayer = 0 a sub-step's outputs are byte-identical to those of a context that was never configured for PBL."""
import numpy as np
import pytest

import pbl_oracle as P
from icar_amd import pbl
from icar_amd.options import options_t
from icar_amd.microphysics import mp_init, mp_var_request
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import substep, step, mp_and_halo
from icar_amd.capi import lib, check
from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kMP_SB04, kPBL_SIMPLE
from util import bits_equal, nbitdiff, parity_record, roughen_winds, MEMBER

pytestmark = pytest.mark.gpu
ADV_ORDER = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
OUTPUTS = [MEMBER[n] for n in ADV_ORDER] + ["u", "v", "w", "pressure", "exner", "density", "temperature", "u_mass", "v_mass", "w_real",
                                             "pressure_interface", "accumulated_precipitation"]


def step_case(oracle, nx, ny, nz, seed, amp):
    """a PBL case whose winds are sheared by noise (u_mass / v_mass come from diagnostic_update in the loop): u varies with (j, k)
    only and v with (k, i) only, so that the noise adds no horizontal divergence (w, rebalanced, and with it the CFL step stay
    moderate); the rows' amplitudes differ, and so do their sub-step counts"""
    c = P.make_case(nx, ny, nz, seed=seed, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=5000.0)      # (a CFL step of 100 s and more)
    c["water_vapor"] = (c["water_vapor"] * np.float32(1.35)).astype(np.float32)
    rng = np.random.default_rng(seed)
    rows = (rng.random((ny, 1, 1)) ** 2).astype(np.float32)                   # calm and rough rows
    c["u"] = (c["u"] + amp * rows * rng.standard_normal((ny, nz, 1))).astype(np.float32)
    c["v"] = (c["v"] + 0.25 * amp * rng.standard_normal((1, nz, nx))).astype(np.float32)
    c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
    dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
    dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(np.float32) for k, sc in dq.items()}
    return c, dq


def options(c, scheme, boundarylayer):
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = scheme
    opt.physics.boundarylayer = boundarylayer
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt)
    return opt


def domain(c, dq, opt):
    d = P.device_domain(c)
    mp_init(opt, d); adv_init(d, opt); pbl.pbl_init(d, opt)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


@pytest.mark.parametrize("scheme", [kMP_THOMPSON, kMP_SB04], ids=["thompson", "mp_simple"])
def test_substep_equals_the_plain_sequence(oracle, scheme):
    nx, ny, nz, dt = 80, 48, 40, 80.0
    c, dq = step_case(oracle, nx, ny, nz, seed=31, amp=12.0)
    opt = options(c, scheme, kPBL_SIMPLE)
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    counts = set()
    for n in range(2):
        substep(a, opt, dt, forced=FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474
        pbl.pbl(b, opt, dt)                                                   # :494
        counts |= set(pbl.nsubsteps(b)[1:-1].tolist())
        mp_and_halo(b, opt, dt)                                               # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, FORCED)                                           # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in OUTPUTS:
            x, y = a.get(m), b.get(m)
            assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), f"sub-step {n + 1}: {m}"
    assert len(counts) >= 2, f"rows with different sub-step counts wanted, got {counts}"
    # ... and the scheme did run inside the sub-step: without it the result is another one
    o = options(c, scheme, 0)
    e = domain(c, dq, o)
    substep(e, o, dt, forced=FORCED, diagnostics=True)
    e.model_time_seconds += dt
    substep(e, o, dt, forced=FORCED, diagnostics=True)
    assert not np.array_equal(e.get("potential_temperature"), a.get("potential_temperature"))
    parity_record("pbl_step", f"substep_vs_plain_sequence/{'thompson' if scheme == kMP_THOMPSON else 'mp_simple'}", {"fields": len(OUTPUTS), "bitdiff_cells": 0, "nsubsteps": sorted(int(x) for x in counts)})
    for d in (a, b, e):
        d.close()


def test_pbl_off_is_byte_identical_to_never_configured(oracle):
    nx, ny, nz, dt = 80, 48, 40, 80.0
    c, dq = step_case(oracle, nx, ny, nz, seed=32, amp=12.0)
    opt = options(c, kMP_THOMPSON, 0)
    never = P.device_domain(c)
    mp_init(opt, never); adv_init(never, opt)
    for k, x in dq.items():
        never.set_dqdt(k, x)
    was_on = domain(c, dq, options(c, kMP_THOMPSON, kPBL_SIMPLE))             # configured for PBL ...
    pbl.pbl_finalize(opt, was_on)                                             # ... and switched off again
    for n in range(2):
        for d in (never, was_on):
            substep(d, opt, dt, forced=FORCED, diagnostics=True)
            d.model_time_seconds += dt
    for m in OUTPUTS:
        assert never.get(m).tobytes() == was_on.get(m).tobytes(), m
    on = domain(c, dq, options(c, kMP_THOMPSON, kPBL_SIMPLE))
    substep(on, options(c, kMP_THOMPSON, kPBL_SIMPLE), dt, forced=FORCED, diagnostics=True)
    substep(on, options(c, kMP_THOMPSON, kPBL_SIMPLE), dt, forced=FORCED, diagnostics=True)
    assert on.get("potential_temperature").tobytes() != never.get("potential_temperature").tobytes(), "with the scheme on the result differs"
    for d in (never, was_on, on):
        d.close()


def test_whole_step_loop_with_pbl_equals_cpu_chain(th_oracle, oracle):
    """icar_hip_step: update_dt -> diagnostic_update -> pbl -> Thompson -> MPDATA (exact mode) -> apply_forcing -> enforce_limits in
    the last two sub-steps, forced winds and pressure (every sub-step its own dt), against the same loop on the CPU"""
    nx, ny, nz = 96, 64, 40
    c, dq = step_case(oracle, nx, ny, nz, seed=33, amp=12.0)
    opt = options(c, kMP_THOMPSON, kPBL_SIMPLE)
    d = P.device_domain(c)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    mp_init(opt, d); adv_init(d, opt); pbl.pbl_init(d, opt)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    f32 = np.float32
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    end = 6.4 * dt0
    n_dev = step(d, end, opt, forced=FORCED, diagnostics=True)
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, dts, t_mp, counts = 0.0, 0, [], None, set()
    while t < end:                                                                                      # time_step.f90:462
        dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
        if t + dt > end: dt = end - t
        enforce = (end - t) < dt * 2
        dt4 = float(f32(dt))
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        if dt > 1e-3:                                                                                   # :483, :494
            nsub, _ = P.simple_pbl({k: s[k] for k in P.SCALARS}, diag["u_mass"], diag["v_mass"], diag["exner"], diag["density"], c["z"], c["dz_mass"],
                                   c["terrain"], c["land_mask"], 2, nx - 1, 2, ny - 1, 1, nz, dt4)
            counts |= set(nsub[1:-1].tolist())
        z = [np.zeros((ny, nx), np.float32) for _ in range(5)]
        mp_dt = dt4 if t_mp is None else float(f32(t - t_mp)); t_mp = t
        th_oracle.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"],
                           s["rain_number"], s["potential_temperature"], diag["exner"], s["pressure"], c["dz_mass"], mp_dt, *z,
                           1, nx, 1, ny, 1, nz, 2, nx - 1, 2, ny - 1, 1, nz)
        acc += z[0]
        q = np.stack([s[n] for n in ADV_ORDER]).copy()
        oracle.advect(2, q, s["u"], s["v"], s["w"], diag["density"], c["jacobian"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"],
                      c["advection_dz"], c["dz_levels"], float(c["dx"]), dt4)
        for m, n in enumerate(ADV_ORDER): s[n] = q[m].copy()
        for n, fb in FORCED:
            oracle.apply_forcing(s[n], dq[n], dt, int(fb), 1, 1, 1, 1)
        if enforce:
            for n in ADV_ORDER: oracle.enforce_limits(s[n])
        t += dt; n_cpu += 1; dts.append(dt)
    assert n_dev == n_cpu and n_cpu >= 6, (n_dev, n_cpu)
    assert all(np.isfinite(a).all() for a in s.values()) and float(s["potential_temperature"].max()) < 600.0
    assert len(counts) >= 2, counts
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    assert bits_equal(d.get("exner"), diag["exner"]) and bits_equal(d.get("density"), diag["density"])
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    assert len(set(dts)) == len(dts)
    parity_record("pbl_step", f"whole_step_loop/96x64x40/exact_mode_{n_cpu}_substeps", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s} | {"nsubsteps": sorted(int(x) for x in counts)})
    d.close()

"""The radiation slot of the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:488):
* icar_hip_step over six or more sub-steps with radiation on, a calendar set, forced winds and icar_hip_mpdata_exact == the same
  loop assembled call by call on the CPU from the oracle's operators and the radiation restatement, every prognostic field and
  the three radiation results bit for bit -- once in mid-year, once with the year's end inside the step;
* icar_hip_substep with the scheme configured == the plain sequence diagnostic_update -> rad -> mp_and_halo -> advect ->
  apply_forcing issued call by call;
* with radiation = 0 a sub-step's outputs are byte-identical to those of a context that was never configured for it."""
import numpy as np
import pytest

import pbl_oracle as P
import ra_oracle as R
from icar_amd import radiation
from icar_amd.options import options_t
from icar_amd.microphysics import mp_init, mp_var_request
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import substep, step, mp_and_halo
from icar_amd.capi import lib, check, IcarHipError
from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kRA_SIMPLE
from util import bits_equal, nbitdiff, parity_record, MEMBER

pytestmark = pytest.mark.gpu
ADV_ORDER = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
OUTPUTS = [MEMBER[n] for n in ADV_ORDER] + ["u", "v", "w", "pressure", "exner", "density", "temperature", "u_mass", "v_mass", "w_real",
                                             "pressure_interface", "accumulated_precipitation"]
NX, NY, NZ = 66, 36, 24


def step_case(oracle, seed):
    """the boundary-layer step case (sheared winds without horizontal divergence, forcing tendencies) with latitudes -90 .. 90
    along j, longitudes -180 .. 360 along i and small hydrometeor fields"""
    c = P.make_case(NX, NY, NZ, seed=seed, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=5000.0)
    c["water_vapor"] = (c["water_vapor"] * np.float32(1.35)).astype(np.float32)
    rng = np.random.default_rng(seed)
    c["u"] = (c["u"] + 6.0 * rng.standard_normal((NY, NZ, 1))).astype(np.float32)
    c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, NZ, NX))).astype(np.float32)
    c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
    c["latitude"] = (np.linspace(-90.0, 90.0, NY)[:, None] + np.zeros((1, NX))).astype(np.float32)
    c["longitude"] = (np.linspace(-180.0, 360.0, NX)[None, :] + rng.uniform(-2, 2, (NY, NX))).clip(-180, 360).astype(np.float32)
    dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
    dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(np.float32) for k, sc in dq.items()}
    return c, dq


def options(c, rad):
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON
    opt.physics.radiation = rad
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt); radiation.ra_var_request(opt)
    return opt


def domain(c, dq, opt, anchor=None):
    d = P.device_domain(c)
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((NY, NX), R.SENTINEL, np.float32))
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt)
    if anchor is not None:
        radiation.rad_calendar(d, *anchor)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def day_of_year(t, anchor):
    """what the library forms at the start of a sub-step (include/icar_hip.h: icar_hip_rad_calendar)"""
    cal, start, yd, nyd = anchor
    D = (t - start) / 86400.0
    if D >= yd:
        D, yd = D - yd, nyd
    return D, yd


@pytest.mark.parametrize("anchor", [(R.GREGORIAN, -(80 * 86400.0 + 30000.0), 365.0, 365.0), (R.GREGORIAN, -(365 * 86400.0 - 150.0), 365.0, 366.0),
                                    (R.THREESIXTY, -(200 * 86400.0 + 70000.0), 360.0, 360.0)], ids=["midyear", "newyear", "360day"])
def test_whole_step_loop_with_radiation_equals_cpu_chain(th_oracle, oracle, anchor):
    """icar_hip_step: update_dt -> diagnostic_update -> rad -> Thompson -> MPDATA (exact mode) -> apply_forcing -> enforce_limits in
    the last two sub-steps, forced winds and pressure (every sub-step its own dt), against the same loop on the CPU"""
    nx, ny, nz = NX, NY, NZ
    c, dq = step_case(oracle, seed=41)
    opt = options(c, kRA_SIMPLE)
    d = domain(c, dq, opt, anchor)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    f32 = np.float32
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    end = 6.4 * dt0
    n_dev = step(d, end, opt, forced=FORCED, diagnostics=True)
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, t_mp, years = 0.0, 0, None, set()
    while t < end:                                                                                      # time_step.f90:462
        dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
        if t + dt > end: dt = end - t
        enforce = (end - t) < dt * 2
        dt4 = float(f32(dt))
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        if dt > 1e-3:                                                                                   # :483, :488
            D, yd = day_of_year(t, anchor); years.add(yd)
            A = dict(rad2d); A["potential_temperature"] = s["potential_temperature"]
            inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
            R.ra_simple(A, inputs, D, yd, anchor[0], dt4, 2, nx - 1, 2, ny - 1, 1, nz)
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
        t += dt; n_cpu += 1
    assert n_dev == n_cpu and n_cpu >= 6, (n_dev, n_cpu)
    assert all(np.isfinite(a).all() for a in s.values())
    assert len(years) == (2 if anchor[3] != anchor[2] else 1), f"the year's end inside the step: {years}"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    for k in R.OUTPUTS[1:]:
        got = d.get(k)
        assert bits_equal(got, rad2d[k]), f"{k}: {nbitdiff(got, rad2d[k])} of {got.size} cells differ"
    m, _ = R.tile_mask(c)
    sw = rad2d["shortwave"][m]
    assert (sw == 0).any() and (sw > 100).any(), "day and night columns"
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    parity_record("ra_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps/{anchor[0]}_{anchor[2]:.0f}", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s})
    d.close()


def test_substep_equals_the_plain_sequence_and_needs_a_calendar(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=42)
    opt = options(c, kRA_SIMPLE)
    anchor = (R.NOLEAP, -(100 * 86400.0 + 40000.0), 365.0, 365.0)
    nocal = domain(c, dq, opt)
    with pytest.raises(IcarHipError, match="calendar"):
        radiation.rad(nocal, opt, dt)
    nocal.close()
    a, b = domain(c, dq, opt, anchor), domain(c, dq, opt, anchor)
    for n in range(2):
        substep(a, opt, dt, forced=FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474
        radiation.rad(b, opt, dt)                                             # :488
        mp_and_halo(b, opt, dt)                                               # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, FORCED)                                           # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in OUTPUTS + R.OUTPUTS[1:]:
            assert a.get(m).tobytes() == b.get(m).tobytes(), f"sub-step {n + 1}: {m}"
    for d in (a, b):
        d.close()


def test_radiation_off_is_byte_identical_to_never_configured(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=43)
    opt = options(c, 0)
    never = P.device_domain(c)
    mp_init(opt, never); adv_init(never, opt)
    for k, x in dq.items():
        never.set_dqdt(k, x)
    anchor = (R.GREGORIAN, -(100 * 86400.0), 365.0, 365.0)
    was_on = domain(c, dq, options(c, kRA_SIMPLE), anchor)                    # configured for radiation ...
    radiation.rad_finalize(opt, was_on)                                       # ... and switched off again
    for n in range(2):
        for d in (never, was_on):
            substep(d, opt, dt, forced=FORCED, diagnostics=True)
            d.model_time_seconds += dt
    for m in OUTPUTS:
        assert never.get(m).tobytes() == was_on.get(m).tobytes(), m
    assert (was_on.get("shortwave") == np.float32(R.SENTINEL)).all(), "nothing ran"
    on = domain(c, dq, options(c, kRA_SIMPLE), anchor)
    for n in range(2):
        substep(on, options(c, kRA_SIMPLE), dt, forced=FORCED, diagnostics=True)
        on.model_time_seconds += dt
    assert on.get("potential_temperature").tobytes() != never.get("potential_temperature").tobytes(), "with the scheme on the result differs"
    for d in (never, was_on, on):
        d.close()

"""The surface-flux slot of the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:491):
* icar_hip_step over six or more sub-steps with rad + lsm + pbl + Thompson + MPDATA (exact mode) on, forced winds, and an update
  gate that is shut for some sub-steps and opens again in the middle of the call == the same loop assembled call by call on the CPU
  from the oracle's operators and the three restatements, every prognostic field and every surface field bit for bit;
* icar_hip_substep with the slot configured == the plain sequence issued call by call;
* with landsurface = 0 and every surface field uploaded (roughness_z0 aside: that one switches the 10 m diagnostics on, as in the
  reference) a sub-step's outputs are byte-identical to those of a context that never heard of the slot; with roughness_z0 uploaded
  too they still are, and only u_10m / v_10m / ustar are new."""
import numpy as np
import pytest

import pbl_oracle as P
import ra_oracle as R
import sfc_oracle as S
from icar_amd import radiation, pbl, surface
from icar_amd.options import options_t
from icar_amd.microphysics import mp_init, mp_var_request
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import substep, step, mp_and_halo
from icar_amd.capi import lib, check
from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kRA_SIMPLE, kPBL_SIMPLE, kLSM_BASIC, kWATER_SIMPLE
from util import bits_equal, nbitdiff, parity_record, MEMBER

pytestmark = pytest.mark.gpu
ADV_ORDER = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
OUTPUTS = [MEMBER[n] for n in ADV_ORDER] + ["u", "v", "w", "pressure", "exner", "density", "temperature", "u_mass", "v_mass", "w_real",
                                             "pressure_interface", "accumulated_precipitation"]
SFC2 = ["sst", "skin_temperature", "sensible_heat", "latent_heat"]
NX, NY, NZ = 66, 20, 16
ANCHOR = (R.GREGORIAN, -(80 * 86400.0 + 30000.0), 365.0, 365.0)


def step_case(oracle, seed):
    """the boundary-layer step case with latitudes and longitudes for the radiation and a surface description: half the cells water,
    sea-surface temperatures around the air's, prescribed fluxes over land, dz_interface = dz_mass"""
    c = P.make_case(NX, NY, NZ, seed=seed, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=5000.0, water=0.5)
    c["water_vapor"] = (c["water_vapor"] * np.float32(1.35)).astype(np.float32)
    rng = np.random.default_rng(seed)
    c["u"] = (c["u"] + 6.0 * rng.standard_normal((NY, NZ, 1))).astype(np.float32)
    c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, NZ, NX))).astype(np.float32)
    c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
    c["latitude"] = (np.linspace(-90.0, 90.0, NY)[:, None] + np.zeros((1, NX))).astype(np.float32)
    c["longitude"] = (np.linspace(-180.0, 360.0, NX)[None, :] + rng.uniform(-2, 2, (NY, NX))).clip(-180, 360).astype(np.float32)
    T0 = (c["potential_temperature"] * c["exner"])[:, 0, :]
    c["sst"] = (T0 + rng.uniform(-5, 5, (NY, NX))).astype(np.float32)
    c["skin_temperature"] = (T0 + rng.uniform(-2, 2, (NY, NX))).astype(np.float32)
    c["sensible_heat"] = rng.uniform(-50, 300, (NY, NX)).astype(np.float32)
    c["latent_heat"] = rng.uniform(-20, 200, (NY, NX)).astype(np.float32)
    c["roughness_z0"] = (10.0 ** rng.uniform(-3, -0.5, (NY, NX))).astype(np.float32)
    c["dz_interface"] = c["dz_mass"].copy()
    dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
    dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(np.float32) for k, sc in dq.items()}
    return c, dq


def options(c, on, update_interval=300):
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON
    if on:
        opt.physics.radiation, opt.physics.boundarylayer = kRA_SIMPLE, kPBL_SIMPLE
        opt.physics.landsurface, opt.physics.watersurface = kLSM_BASIC, kWATER_SIMPLE
    opt.lsm_options.update_interval = update_interval
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt); radiation.ra_var_request(opt); pbl.pbl_var_request(opt); surface.lsm_var_request(opt)
    return opt


def domain(c, dq, opt, roughness=True):
    d = P.device_domain({k: v for k, v in c.items() if roughness or k != "roughness_z0"})
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((NY, NX), R.SENTINEL, np.float32))
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt); surface.lsm_init(d, opt)
    radiation.rad_calendar(d, *ANCHOR)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def day_of_year(t):
    cal, start, yd, nyd = ANCHOR
    D = (t - start) / 86400.0
    return (D - yd, nyd) if D >= yd else (D, yd)


def test_whole_step_loop_with_every_slot_equals_cpu_chain(th_oracle, oracle):
    nx, ny, nz = NX, NY, NZ
    c, dq = step_case(oracle, seed=51)
    f32 = np.float32
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    ui = max(int(2.5 * dt0), 1)                                       # shut for two sub-steps or so, then open again inside the call
    opt = options(c, True, update_interval=ui)
    d = domain(c, dq, opt)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    end = 6.4 * dt0
    n_dev = step(d, end, opt, forced=FORCED, diagnostics=True)
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
    sfc = {k: c[k].copy() for k in ("roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")}
    sfc.update(u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32),
               qsfc=c["water_vapor"][:, 0, :].copy(), qfx=np.zeros((ny, nx), f32), last_model_time=-999.0)
    par = dict(watersurface=kWATER_SIMPLE, landsurface=kLSM_BASIC, sfc_layer_thickness=400.0, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0,
               update_interval=ui, kts=1)
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, t_mp, gates = 0.0, 0, None, []
    while t < end:                                                                                      # time_step.f90:462
        dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
        if t + dt > end: dt = end - t
        enforce = (end - t) < dt * 2
        dt4 = float(f32(dt))
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        cc = dict(par, density=diag["density"], exner=diag["exner"], temperature=diag["temperature"], u_mass=diag["u_mass"], v_mass=diag["v_mass"],
                  surface_pressure=diag["surface_pressure"], z=c["z"], terrain=c["terrain"], sst=c["sst"], land_mask=c["land_mask"], dz_interface=c["dz_interface"])
        A = dict(sfc, potential_temperature=s["potential_temperature"], water_vapor=s["water_vapor"])
        S.diag_10m(cc, A)                                                                               # :143-161
        if dt > 1e-3:                                                                                   # :483
            D, yd = day_of_year(t)                                                                      # :488 rad
            Ar = dict(rad2d); Ar["potential_temperature"] = s["potential_temperature"]
            inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
            R.ra_simple(Ar, inputs, D, yd, ANCHOR[0], dt4, 2, nx - 1, 2, ny - 1, 1, nz)
            is_open = S.gate(cc, A, t)                                                                  # :491 lsm
            if is_open: S.water_simple(cc, A)
            gates.append(is_open)
            S.apply_fluxes(cc, A, dt4)
            sfc["last_model_time"] = A["last_model_time"]
            P.simple_pbl({k: s[k] for k in P.SCALARS}, diag["u_mass"], diag["v_mass"], diag["exner"], diag["density"], c["z"], c["dz_mass"],   # :494 pbl
                         c["terrain"], c["land_mask"], 2, nx - 1, 2, ny - 1, 1, nz, dt4)
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
    assert gates[0] and False in gates and True in gates[gates.index(False):], f"the gate: open, shut, open again inside the call: {gates}"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        print(n, "differing cells:", nbitdiff(got, s[n]))
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    for k in S.STATE2:
        got = d.get(k)
        assert bits_equal(got, sfc[k]), f"{k}: {nbitdiff(got, sfc[k])} of {got.size} cells differ"
    for k in R.OUTPUTS[1:]:
        assert bits_equal(d.get(k), rad2d[k]), k
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    parity_record("sfc_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s})
    d.close()


def test_substep_equals_the_plain_sequence(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=52)
    opt = options(c, True, update_interval=100)
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    for n in range(3):
        substep(a, opt, dt, forced=FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474, the 10 m winds included
        radiation.rad(b, opt, dt)                                             # :488
        surface.lsm(b, opt, dt)                                               # :491
        pbl.pbl(b, opt, dt)                                                   # :494
        _mp_and_halo_keeping_the_gate(b, opt, dt)                             # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, FORCED)                                           # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in OUTPUTS + R.OUTPUTS[1:] + S.STATE2:
            assert a.get(m).tobytes() == b.get(m).tobytes(), f"sub-step {n + 1}: {m}"
    for d in (a, b):
        d.close()


def _mp_and_halo_keeping_the_gate(d, opt, dt):
    """time_step.mp_and_halo switches the surface slot off for its one library call, which resets lsm's update gate like lsm_init
    does; the plain sequence wants the gate carried, so the block is issued through the pieces that leave it alone"""
    from icar_amd.microphysics import mp
    mp(d, opt, dt, halo=1)
    d.halo_send()
    mp(d, opt, dt, subset=1)
    d.halo_retrieve()


def test_landsurface_0_is_byte_identical_to_never_configured(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=53)
    opt = options(c, False)
    bare = {k: v for k, v in c.items() if k not in SFC2 + ["roughness_z0", "dz_interface"]}
    never = P.device_domain(bare)
    mp_init(opt, never); adv_init(never, opt)
    for k, x in dq.items():
        never.set_dqdt(k, x)
    loaded = domain(c, dq, opt, roughness=False)                              # every surface field but roughness_z0, landsurface = 0
    rough = domain(c, dq, opt, roughness=True)                                # ... and with it: the 10 m diagnostics run, nothing else changes
    was_on = domain(c, dq, options(c, True))
    radiation.rad_finalize(opt, was_on); pbl.pbl_finalize(opt, was_on); surface.lsm_finalize(opt, was_on)
    for n in range(2):
        for d in (never, loaded, rough, was_on):
            substep(d, opt, dt, forced=FORCED, diagnostics=True)
            d.model_time_seconds += dt
    for m in OUTPUTS:
        ref = never.get(m).tobytes()
        assert loaded.get(m).tobytes() == ref and rough.get(m).tobytes() == ref and was_on.get(m).tobytes() == ref, m
    for k in SFC2:
        assert loaded.get(k).tobytes() == c[k].tobytes() and rough.get(k).tobytes() == c[k].tobytes(), f"{k}: nothing ran"
    assert rough.get("roughness_z0").tobytes() == c["roughness_z0"].tobytes()
    assert float(np.abs(rough.get("u_10m")[1:-1, 1:-1]).min()) > 0 and not (rough.get("ustar")[1:-1, 1:-1] == np.float32(0.1)).all()
    on = domain(c, dq, options(c, True))
    for n in range(2):
        substep(on, options(c, True), dt, forced=FORCED, diagnostics=True)
        on.model_time_seconds += dt
    assert on.get("water_vapor").tobytes() != never.get("water_vapor").tobytes(), "with the slot on the result differs"
    for d in (never, loaded, rough, was_on, on):
        d.close()

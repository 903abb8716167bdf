"""Diagnostics where they can be observed (icar_amd/csrc/timestep.hip: lazy_diag_part).

icar_hip_step / icar_hip_step_n run many sub-steps in one library call; a sub-step that is not the call's last writes only the
diagnostics something on the device reads before the next diagnostic_update (exner always; density for the schemes that read it;
everything with a boundary layer, advect_density, column integrals on the device or WSM3).  What the caller can see must not
change:
* step_n(4) == four step_n(1) from the same start, every field the library can download byte for byte (the eight diagnostic
  fields included), for Thompson + MPDATA, mp_simple + upwind and WSM6 + MPDATA;
* icar_hip_step to an end time that clamps the last sub-step == the same sub-steps issued one at a time;
* the configurations that keep per-sub-step diagnostics (boundary layer, advect_density, column integrals, WSM3) likewise: a
  reader that was wrongly skipped shows here;
* no diagnostic field keeps a stale value: filled with a sentinel before step_n(3), only the cells that no single sub-step writes
  either (the ring of w_real) still hold it."""
import numpy as np
import pytest

import pbl_oracle as P
from icar_amd import pbl
from icar_amd import _fields as F
from icar_amd.capi import IcarHipError
from icar_amd.options import options_t
from icar_amd.microphysics import mp_init, mp_var_request
from icar_amd.advection import adv_init
from icar_amd.time_step import substep, step, step_n, update_dt
from icar_amd.constants import kADV_MPDATA, kADV_UPWIND, kMP_THOMPSON, kMP_SB04, kMP_WSM6, kMP_WSM3, kPBL_SIMPLE

pytestmark = pytest.mark.gpu
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
DIAGNOSTICS = ["temperature", "density", "pressure_interface", "surface_pressure", "temperature_interface", "u_mass", "v_mass", "w_real"]
TILES = [(24, 10, 16), (67, 7, 9)]
SENTINEL = -12345.0
_cases = {}


def case(oracle, nx, ny, nz):
    """sheared, noisy winds (every sub-step has its own dt once they are forced), slopes for w_real, tendencies for the forcing"""
    if (nx, ny, nz) not in _cases:
        c = P.make_case(nx, ny, nz, seed=41, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=2000.0)      # (a CFL step of ~60 s: under the 120 s cap)
        c["water_vapor"] = (c["water_vapor"] * np.float32(1.35)).astype(np.float32)
        rng = np.random.default_rng(41)
        c["u"] = (c["u"] + 6.0 * rng.standard_normal((ny, nz, 1))).astype(np.float32)
        c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, nz, nx))).astype(np.float32)
        c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
        c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
        c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
        dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
        dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(np.float32) for k, sc in dq.items()}
        _cases[(nx, ny, nz)] = (c, dq)
    return _cases[(nx, ny, nz)]


def options(c, adv, scheme, boundarylayer=0, advect_density=False):
    opt = options_t(); opt.physics.advection = adv; opt.physics.microphysics = scheme
    opt.physics.boundarylayer = boundarylayer
    opt.parameters.advect_density = advect_density
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt)
    return opt


def domain(c, dq, opt, columns=False, sentinel=False):
    d = P.device_domain(c)
    mp_init(opt, d); adv_init(d, opt)
    if opt.physics.boundarylayer:
        pbl.pbl_init(d, opt)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    if columns:
        for n in ("ivt", "iwv", "iwl", "iwi"):
            d.set(n, np.zeros((c["ny"], c["nx"]), np.float32))
    if sentinel:
        for n in DIAGNOSTICS:
            d.fill(n, SENTINEL)
    return d


def downloads(d):
    """every field the library hands out, as bytes"""
    out = {}
    for n in F.NAMES:
        try:
            out[n] = d.get(n).tobytes()
        except IcarHipError:
            pass
    return out


def assert_same_state(a, b, what):
    x, y = downloads(a), downloads(b)
    assert set(x) == set(y), (what, sorted(set(x) ^ set(y)))
    assert all(n in x for n in DIAGNOSTICS + ["exner"]), what
    bad = [n for n in x if x[n] != y[n]]
    assert not bad, f"{what}: {bad} differ"
    assert a.model_time_seconds == b.model_time_seconds, what


CONFIGS = {"thompson_mpdata": (kADV_MPDATA, kMP_THOMPSON), "mp_simple_upwind": (kADV_UPWIND, kMP_SB04), "wsm6_mpdata": (kADV_MPDATA, kMP_WSM6)}


@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_step_n_equals_single_sub_steps(oracle, config, tile):
    c, dq = case(oracle, *tile)
    opt = options(c, *CONFIGS[config])
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    step_n(a, 4, opt, forced=FORCED)
    dts = [step_n(b, 1, opt, forced=FORCED) for _ in range(4)]
    assert len(set(dts)) == 4, "every sub-step its own dt wanted"
    assert_same_state(a, b, f"{config} {tile}")
    a.close(); b.close()


@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("config", ["thompson_mpdata", "mp_simple_upwind"])
def test_step_to_a_clamping_end_time_equals_single_sub_steps(oracle, config, tile):
    c, dq = case(oracle, *tile)
    opt = options(c, *CONFIGS[config])
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    b.configure(opt, forced=FORCED, diagnostics=True, prefetch_dt=True)
    end = 6.4 * update_dt(b, opt)                                             # (far enough for sub-steps that open ahead of update_dt)
    n = step(a, end, opt, forced=FORCED)
    t, m, clamped = 0.0, 0, False
    while t < end:                                                            # time_step.f90:462-547
        dt = update_dt(b, opt)
        if t + dt > end:
            dt = end - t; clamped = True
        substep(b, opt, dt, forced=FORCED, enforce=(end - t) < dt * 2)
        t = t + dt; m += 1
        b.model_time_seconds = t
    assert n == m and m >= 6 and clamped, (n, m, clamped)
    assert_same_state(a, b, f"step {config} {tile}")
    a.close(); b.close()


KEEPERS = {"boundary_layer": dict(scheme=kMP_THOMPSON, boundarylayer=kPBL_SIMPLE), "advect_density": dict(scheme=kMP_THOMPSON, advect_density=True),
           "column_integrals": dict(scheme=kMP_THOMPSON, columns=True), "wsm3": dict(scheme=kMP_WSM3)}


@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("config", list(KEEPERS))
def test_configurations_that_keep_their_diagnostics(oracle, config, tile):
    c, dq = case(oracle, *tile)
    k = dict(KEEPERS[config]); columns = k.pop("columns", False)
    opt = options(c, kADV_MPDATA, k.pop("scheme"), **k)
    a, b = domain(c, dq, opt, columns=columns), domain(c, dq, opt, columns=columns)
    step_n(a, 3, opt, forced=FORCED)
    for _ in range(3):
        step_n(b, 1, opt, forced=FORCED)
    assert_same_state(a, b, f"{config} {tile}")
    if columns:
        assert float(a.get("iwv").max()) > 0.0
    a.close(); b.close()


@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t)))
def test_no_stale_diagnostic_survives(oracle, tile):
    c, dq = case(oracle, *tile)
    opt = options(c, kADV_MPDATA, kMP_THOMPSON)
    a, b, one = (domain(c, dq, opt, sentinel=True) for _ in range(3))
    step_n(a, 3, opt, forced=FORCED)
    for _ in range(3):
        step_n(b, 1, opt, forced=FORCED)
    step_n(one, 1, opt, forced=FORCED)
    for n in DIAGNOSTICS:
        x, never = a.get(n), one.get(n) == np.float32(SENTINEL)               # the cells that a single sub-step leaves alone, too
        assert np.array_equal(x == np.float32(SENTINEL), never), n
        assert not never.any() or n == "w_real", n                            # (w_real is defined on the interior columns only)
        assert x.tobytes() == b.get(n).tobytes(), n
    assert_same_state(a, b, f"sentinel {tile}")
    for d in (a, b, one):
        d.close()

"""The clock and gate bookkeeping of the step loops (icar_amd/csrc/timestep.hip: icar_mp_run inside icar_substep) with
mp_update_interval > 0: a microphysics gate that opens and shuts inside icar_hip_step / icar_hip_step_n.

The interior pass is issued before the strips and mp_last_model_time is put back for them; with Thompson alone a sub-step that is not
the call's last launches no diagnostic kernel, gate shut or not.  Against the loop on the host with a gate written from
mp_driver.f90:692-718 (tests/step_loop_model.py) and against the same sub-steps issued one at a time, bit for bit.  What the cases
must do for this to prove anything is checked on the host by tests/test_step_loop_model_inputs.py."""
import numpy as np
import pytest

import step_loop_model as M
from icar_amd.capi import lib, check
from icar_amd.time_step import substep, step, step_n, update_dt
from test_gpu_lazy_diagnostics import assert_same_state, DIAGNOSTICS, SENTINEL
from util import bits_equal, nbitdiff

pytestmark = pytest.mark.gpu
TILE_IDS = dict(ids=lambda t: "x".join(map(str, t)))


def assert_equals_chain(d, r, config, what):
    """every prognostic field, exner, density, the accumulated precipitation and the clock of the device against the host chain's"""
    scheme = M.CONFIGS[config][0]
    assert r.too_small is None, what
    for k in M.ADVECTED[scheme] + M.WINDS:
        got = d.get(M.DEVICE_NAME[k])
        assert bits_equal(got, r.s[k]), f"{what}: {k}: {nbitdiff(got, r.s[k])} of {got.size} cells differ after {r.n} sub-steps"
    assert bits_equal(d.get("exner"), r.diag["exner"]) and bits_equal(d.get("density"), r.diag["density"]), what
    assert r.acc.max() > 0 and np.array_equal(d.get("accumulated_precipitation"), r.acc), what
    if scheme == "simple":
        assert np.array_equal(d.get("accumulated_snowfall"), r.acc_snow), what
    assert d.model_time_seconds == r.t, (what, d.model_time_seconds, r.t)


def device(oracle, tile, config, which="opens_and_shuts", top=False, halo=None):
    c, dq = M.case(oracle, tile)
    opt = M.device_options(c, config, M.interval(oracle, c, which), M.top_level(c) if top else 0)
    return c, opt, M.device_domain(c, dq, opt, halo=halo)


@pytest.mark.parametrize("tile", M.TILES, **TILE_IDS)
@pytest.mark.parametrize("which", list(M.INTERVALS))
@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_step_with_a_gate_equals_the_host_chain(th_oracle, config, which, tile):
    c, opt, d = device(th_oracle, tile, config, which)
    n = step(d, M.end_time(th_oracle, c), opt, forced=M.FORCED)
    r = M.chain(th_oracle, tile, config, which)
    assert n == r.n, (n, r.n)
    assert_equals_chain(d, r, config, f"{config} {which} {tile}")
    d.close()


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_top_mp_level_in_the_loop(th_oracle, config):
    tile = M.TILES[0]
    c, opt, d = device(th_oracle, tile, config, top=True)
    n = step(d, M.end_time(th_oracle, c), opt, forced=M.FORCED)
    r, plain = M.chain(th_oracle, tile, config, top=True), M.chain(th_oracle, tile, config)
    assert n == r.n
    assert_equals_chain(d, r, config, f"top_mp_level {config}")
    assert any(not np.array_equal(d.get(M.DEVICE_NAME[k]), plain.s[k]) for k in M.ADVECTED[M.CONFIGS[config][0]]), "top_mp_level must matter"
    d.close()


def single_sub_steps(d, opt, nsteps=None, end=None):
    """the loop of icar_hip_step_n (nsteps) or icar_hip_step (end) with one library call per operation and the clock kept by the host"""
    t, dts = d.model_time_seconds, []
    while (len(dts) < nsteps) if end is None else (t < end):                  # time_step.f90:462-547
        dt = update_dt(d, opt)
        dts.append(dt)
        if end is not None and t + dt > end:
            dt = end - t
        substep(d, opt, dt, forced=M.FORCED, enforce=end is not None and (end - t) < dt * 2)
        t = t + dt
        d.model_time_seconds = t
    return dts


@pytest.mark.parametrize("mode", ["step_n", "step"])
@pytest.mark.parametrize("config", list(M.DEVICE_CONFIGS))
def test_loops_with_a_gate_equal_single_sub_steps(th_oracle, config, mode):
    tile = M.TILES[0]
    c, opt, a = device(th_oracle, tile, config)
    b = device(th_oracle, tile, config)[2]
    if mode == "step_n":
        step_n(a, 5, opt, forced=M.FORCED)
        dts = single_sub_steps(b, opt, nsteps=5)
    else:
        n = step(a, M.end_time(th_oracle, c), opt, forced=M.FORCED)
        dts = single_sub_steps(b, opt, end=M.end_time(th_oracle, c))
        assert n == len(dts)
    assert_same_state(a, b, f"{mode} {config}")
    if config in M.CONFIGS:                                                   # every dt of update_dt is the host chain's
        r = M.chain(th_oracle, tile, config, mode=mode)
        if mode == "step_n":
            assert dts == r.dts[:5], (dts, r.dts)
        else:                                                                 # (the chain records the last sub-step's dt as it was clamped)
            assert dts[:-1] == r.dts[:-1] and r.records[-1].clamped and dts[-1] > r.dts[-1], (dts, r.dts)
    assert len(set(dts)) == len(dts)
    a.close(); b.close()


@pytest.mark.parametrize("nsteps", [4, 5])
def test_no_sentinel_survives_a_gated_loop(th_oracle, nsteps):
    """Thompson alone: sub-steps 1 and 3 run neither a diagnostic launch nor a Thompson launch that makes exner; the call's last
    sub-step has the gate open (5) or shut (4)"""
    tile = M.TILES[0]
    c, opt, a = device(th_oracle, tile, "thompson_mpdata")
    b = device(th_oracle, tile, "thompson_mpdata")[2]
    filled = DIAGNOSTICS + ["exner"]
    for d in (a, b):
        for n in filled:
            d.fill(n, SENTINEL)
    step_n(a, nsteps, opt, forced=M.FORCED)
    single_sub_steps(b, opt, nsteps=nsteps)
    r = M.chain(th_oracle, tile, "thompson_mpdata", mode="step_n")
    assert [x.gate_open for x in r.records[:nsteps]] == [True, False, True, False, True][:nsteps]
    for n in filled:
        x, y = a.get(n), b.get(n)
        assert np.array_equal(x == np.float32(SENTINEL), y == np.float32(SENTINEL)), n
        assert not (y == np.float32(SENTINEL)).any() or n == "w_real", n     # (w_real is defined on the interior columns only)
        assert x.tobytes() == y.tobytes(), n
    assert_same_state(a, b, f"sentinel {nsteps}")
    a.close(); b.close()


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_a_halo_of_two_takes_the_one_stream_order(th_oracle, config):
    tile = M.TILES[0]
    c, opt, d = device(th_oracle, tile, config, halo=2)
    n = step(d, M.end_time(th_oracle, c), opt, forced=M.FORCED)
    r = M.chain(th_oracle, tile, config)
    assert n == r.n
    assert_equals_chain(d, r, config, f"halo 2 {config}")
    d.close()


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_gate_at_a_large_clock(th_oracle, config):
    tile = M.TILES[0]
    c, opt, d = device(th_oracle, tile, config)
    d.model_time_seconds = M.CLOCK_OFFSET
    n = step(d, M.end_time(th_oracle, c, M.CLOCK_OFFSET), opt, forced=M.FORCED)
    r = M.chain(th_oracle, tile, config, t0=M.CLOCK_OFFSET)
    assert n == r.n
    assert_equals_chain(d, r, config, f"clock offset {config}")
    d.close()


@pytest.mark.parametrize("reset", [False, True], ids=["two_calls", "mp_reset_between"])
@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_mp_reset_between_two_step_n_calls(th_oracle, config, reset):
    tile = M.TILES[0]
    c, opt, d = device(th_oracle, tile, config)
    step_n(d, M.RESET_AT, opt, forced=M.FORCED)
    if reset:
        check(lib().icar_hip_mp_reset(d.ctx), "icar_hip_mp_reset")
    dt = step_n(d, M.RESET_STEPS - M.RESET_AT, opt, forced=M.FORCED)
    r = M.chain(th_oracle, tile, config, mode="step_n", reset=reset)
    assert dt == r.dts[-1]
    assert_equals_chain(d, r, config, f"mp_reset {reset} {config}")
    d.close()

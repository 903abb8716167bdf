"""What tests/test_gpu_step_loop_gate.py and tests/test_gpu_step_failed_state.py rest on, checked with the host model alone
(tests/step_loop_model.py): the chosen intervals open and shut the microphysics gate where the GPU tests need it, top_mp_level
matters, the clock offset and icar_hip_mp_reset change what the gate does, and the oversized dqdt of u lets the first sub-step
complete and stops the second.  `pytest -s` prints the gate pattern of every case."""
import numpy as np
import pytest

import step_loop_model as M

f32 = np.float32


def pattern(r):
    return "".join("O" if x.gate_open else "-" for x in r.records)


def test_gate_restates_the_driver():
    """mp_driver.f90:692-718 on numbers worked out by hand (REAL(4) dt, REAL(8) clock)"""
    g = M.Gate(100.0, top_mp_level=17)
    assert g.call(0.0, 40.0, 24, halo=True) == (100.0, 17) and g.last == -100.0        # first call: last = now - max(upd, dt); the halo pass keeps it
    assert g.call(0.0, 40.0, 24, halo=False) == (100.0, 17) and g.last == 0.0
    assert g.call(40.0, 40.0, 24, halo=False) == (None, 24)                            # (40 + 40) - 0 < 100
    assert g.call(80.0, 40.0, 24, halo=False) == (80.0, 17) and g.last == 80.0         # mp_dt is the time since the last run, not dt
    g = M.Gate(0.0)
    assert g.call(5.0, 0.1, 9, halo=False) == (float(f32(0.1)), 9)                     # interval 0, first call: mp_dt = REAL(4) dt
    assert g.call(5.1, 0.1, 9, halo=False) == (float(f32(5.1 - 5.0)), 9)
    g = M.Gate(30.0, top_mp_level=24)
    assert g.call(0.0, 60.0, 24, halo=False) == (60.0, 24)                             # first call: max(upd, dt) = dt; top_mp_level == kte changes nothing
    g.reset()
    assert g.call(60.0, 50.0, 24, halo=False) == (50.0, 24)
    # at a large clock the REAL(4) of the difference is taken, not the difference of REAL(4) clocks
    g = M.Gate(0.0)
    t = M.CLOCK_OFFSET
    g.call(t, 61.3, 9, halo=False)
    assert g.call(t + 61.3, 59.9, 9, halo=False)[0] == float(f32((t + 61.3) - t)) != float(f32(t + 61.3) - f32(t))


@pytest.mark.parametrize("tile", M.TILES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_intervals_open_and_shut_the_gate(th_oracle, config, tile):
    c, _ = M.case(th_oracle, tile)
    dt0 = M.first_dt(th_oracle, c)
    assert 0.1 < dt0 < 120.0, "the case's CFL step lies under the cap"
    runs = {w: M.chain(th_oracle, tile, config, w) for w in M.INTERVALS}
    for w, r in runs.items():
        print(f"\n{config} {tile} {w}: upd = {M.interval(th_oracle, c, w):.3f}, dt0 = {dt0:.3f}, gate {pattern(r)}, "
              f"mp_dt {[None if x.mp_dt is None else round(x.mp_dt, 2) for x in r.records]}")
        assert r.too_small is None and r.n >= 8 and r.records[-1].clamped and not any(x.clamped for x in r.records[:-1]), w
        assert [x.enforce for x in r.records[-2:]] == [True, True] and not any(x.enforce for x in r.records[:-2]), w
        assert r.records[0].dt == dt0 and len(set(r.dts)) == len(r.dts), "forced winds: every sub-step its own dt"
        assert all(np.isfinite(a).all() for a in r.s.values()) and float(r.s["potential_temperature"].max()) < 600.0, "the case stays physical"
        assert r.acc.max() > 0 and float(r.s["cloud_water"].max()) > 1e-6, "the case has active microphysics"
    r = runs["always_open"]
    assert all(x.gate_open for x in r.records)
    assert r.records[0].mp_dt == float(f32(r.records[0].dt)) != M.interval(th_oracle, c, "always_open"), "first mp_dt = dt, not upd"
    r = runs["first_call_only"]
    assert M.interval(th_oracle, c, "first_call_only") > r.t, "an interval longer than the run"
    assert [x.gate_open for x in r.records] == [True] + [False] * (r.n - 1) and r.records[0].mp_dt == M.interval(th_oracle, c, "first_call_only")
    r = runs["opens_and_shuts"]
    o = [x.gate_open for x in r.records]
    assert sum(o) >= 2 and len(o) - sum(o) >= 2, pattern(r)
    # a shut sub-step followed by an open one that is not the call's last: the put-back of last_model_time decides what the strips
    # of that open sub-step see
    assert any(not o[k] and o[k + 1] for k in range(len(o) - 2)), pattern(r)
    assert r.records[0].mp_dt == M.interval(th_oracle, c, "opens_and_shuts")
    later = [x.mp_dt for x in r.records[1:] if x.gate_open]
    assert all(m > 1.5 * dt0 for m in later), "the later calls integrate over more than one sub-step"
    # the three intervals are three different runs
    keys = M.ADVECTED[M.CONFIGS[config][0]]
    for a, b in (("always_open", "opens_and_shuts"), ("opens_and_shuts", "first_call_only")):
        assert any(not np.array_equal(runs[a].s[k], runs[b].s[k]) for k in keys), (a, b)


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_top_mp_level_matters(th_oracle, config):
    tile = M.TILES[0]
    c, _ = M.case(th_oracle, tile)
    assert 0 < M.top_level(c) < c["nz"]
    with_top, without = M.chain(th_oracle, tile, config, top=True), M.chain(th_oracle, tile, config)
    assert pattern(with_top) == pattern(without) and with_top.dts == without.dts
    keys = M.ADVECTED[M.CONFIGS[config][0]]
    assert any(not np.array_equal(with_top.s[k], without.s[k]) for k in keys), "the chain without top_mp_level differs"
    assert with_top.acc.max() > 0


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_clock_offset_case(th_oracle, config):
    tile = M.TILES[0]
    r, zero = M.chain(th_oracle, tile, config, t0=M.CLOCK_OFFSET), M.chain(th_oracle, tile, config)
    o = [x.gate_open for x in r.records]
    assert sum(o) >= 2 and len(o) - sum(o) >= 2 and r.too_small is None and r.records[-1].clamped, pattern(r)
    assert pattern(r) == pattern(zero)
    # at this clock a REAL(4) holds 1/16 s: a gate that rounded the clock before it took the difference would integrate over other times
    now, last, wrong = M.CLOCK_OFFSET, None, 0
    for x in r.records:
        if x.gate_open:
            wrong += last is not None and float(f32(now) - f32(last)) != x.mp_dt
            last = now
        now += x.dt
    assert wrong >= 2 and now == r.t
    assert any(float(f32(x.dt)) != x.dt for x in r.records), "the clamped dt is not a REAL(4): (double)(float)dt differs from dt"


@pytest.mark.parametrize("config", list(M.CONFIGS))
def test_mp_reset_case(th_oracle, config):
    tile = M.TILES[0]
    c, _ = M.case(th_oracle, tile)
    upd = M.interval(th_oracle, c, "opens_and_shuts")
    r, plain = M.chain(th_oracle, tile, config, mode="step_n", reset=True), M.chain(th_oracle, tile, config, mode="step_n")
    print(f"\n{config}: with the reset {pattern(r)}, without {pattern(plain)}")
    assert r.n == plain.n == M.RESET_STEPS and not any(x.enforce or x.clamped for x in r.records)
    x = r.records[M.RESET_AT]
    assert x.gate_open and x.mp_dt == max(upd, float(f32(x.dt))), "the call after the reset is a first one"
    assert plain.records[M.RESET_AT].mp_dt != x.mp_dt, "without the reset that sub-step does something else"
    keys = M.ADVECTED[M.CONFIGS[config][0]]
    assert any(not np.array_equal(r.s[k], plain.s[k]) for k in keys)


@pytest.mark.parametrize("with_nan", [False, True], ids=["too_large", "too_large_and_a_nan"])
def test_oversized_tendency_stops_the_second_sub_step(th_oracle, with_nan):
    tile = M.TILES[0]
    c, dq = M.case(th_oracle, tile)
    bad = M.too_large_tendencies(dq, with_nan)
    assert np.isnan(bad["u"]).sum() == int(with_nan) and np.isfinite(bad["u"]).sum() == bad["u"].size - int(with_nan)
    r = M.run(th_oracle, c, bad, nsteps=4)
    assert r.n == 1 and r.records[0].dt == M.first_dt(th_oracle, c), "the first dt is untouched: the first sub-step completes"
    assert r.too_small is not None and 0.0 < r.too_small < 0.05, "a factor 2 under the reference's 0.1 s stop (time_step.f90:322-328)"
    # (the oracle's max_courant drops a NaN wind as the reference's MAX does, so both variants stop with one finite dt here; the
    # library carries the NaN into its maximum and names it, tests/test_gpu_step_failed_state.py)
    # the state the second update_dt looks at is finite and in range (one NaN where the variant puts it)
    assert np.isfinite(r.s["u"]).sum() == r.s["u"].size - int(with_nan) and float(np.nanmax(np.abs(r.s["u"]))) < 1e6
    assert all(np.isfinite(r.s[k]).all() for k in r.s if k != "u")
    # with a microphysics interval the same happens (the failure with nothing opened)
    g = M.run(th_oracle, c, bad, nsteps=4, update_interval=1.0)
    assert g.n == 1 and g.too_small == r.too_small and g.records[0].gate_open
    # the recovery: three more sub-steps from the first one's state with the sane tendencies
    good = M.run(th_oracle, c, dq, nsteps=1)
    assert good.records[0].dt == r.records[0].dt
    rec = M.run(th_oracle, c, dq, nsteps=3, t0=good.t, state=good.s)
    assert rec.n == 3 and rec.too_small is None and all(x.gate_open for x in rec.records)
    assert rec.records[0].mp_dt == float(f32(rec.records[0].dt)), "after the recovery the microphysics call is a first one: mp_dt = dt"

"""The `failed` state of a context (icar_amd/csrc/timestep.hip: update_dt_opened; include/icar_hip.h, icar_hip_step).

update_dt fails in the second sub-step of icar_hip_step_n: the first sub-step's forcing applies a dqdt of u after which the prefetched
Courant maximum asks for dt < 0.1 s, where the reference stops (time_step.f90:322-328).  With Thompson alone, mp_update_interval 0,
halo_size 1, cfl_strictness 3 and the prefetched dt the second sub-step was opened ahead of update_dt (icar_substep_can_open_early),
so its microphysics has already run: the context is marked failed, every stepping entry point refuses it, and after the fields are
reloaded and the clock set it continues as a newly created context does.  With a microphysics interval nothing is opened early and
the context is not marked.  No kernel runs on anything but finite numbers (one NaN wind in the second variant, which only the
Courant reduction -- it carries a NaN wind into its maximum -- and the mass-point winds read); what is tested is the library's
error return.  The host model's view of the same cases: tests/test_step_loop_model_inputs.py."""
import ctypes

import numpy as np
import pytest

import step_loop_model as M
from icar_amd import _fields as F
from icar_amd.capi import lib, IcarHipError
from icar_amd.time_step import step_n
from test_gpu_lazy_diagnostics import assert_same_state, downloads, DIAGNOSTICS
from util import bits_equal

pytestmark = pytest.mark.gpu
TILE = M.TILES[0]
CONFIG = "thompson_mpdata"
REFUSAL = "abandoned a half-applied sub-step"
VARIANTS = {"too_large": dict(with_nan=False, cause="time step too small"),
            "too_large_and_a_nan": dict(with_nan=True, cause="the CFL maximum is NaN")}


def contexts(oracle, tendencies=None, update_interval=0.0, n=1, tile=TILE):
    c, dq = M.case(oracle, tile)
    opt = M.device_options(c, CONFIG, update_interval)
    ds = [M.device_domain(c, dq if tendencies is None else tendencies, opt) for _ in range(n)]
    return c, dq, opt, ds


def failing(oracle, variant):
    """a context whose step_n(4) has failed in the second sub-step, and the error"""
    c, dq = M.case(oracle, TILE)
    c, dq, opt, (d,) = contexts(oracle, M.too_large_tendencies(dq, VARIANTS[variant]["with_nan"]))
    with pytest.raises(IcarHipError) as e:
        step_n(d, 4, opt, forced=M.FORCED)
    return c, dq, opt, d, str(e.value)


def refused_calls(d):
    """every entry point behind cfg_ok: (name, return code, message)"""
    L, x = lib(), d.ctx
    n, dt, nz, f = ctypes.c_int(), ctypes.c_double(), ctypes.c_int(), ctypes.c_float(30.0)
    calls = [("step", lambda: L.icar_hip_step(x, d.model_time_seconds + 100.0, ctypes.byref(n))),
             ("step_n", lambda: L.icar_hip_step_n(x, 1, ctypes.byref(dt))),
             ("substep", lambda: L.icar_hip_substep(x, 30.0, 0)),
             ("update_dt", lambda: L.icar_hip_update_dt(x, ctypes.byref(dt))),
             ("compute_dt", lambda: L.icar_hip_compute_dt(x, ctypes.byref(dt))),
             ("mp", lambda: L.icar_hip_mp(x, 30.0, -1, -1)),
             ("advect_step", lambda: L.icar_hip_advect_step(x, 30.0)),
             ("pbl", lambda: L.icar_hip_pbl(x, f)),
             ("rad", lambda: L.icar_hip_rad(x, f)),
             ("lsm", lambda: L.icar_hip_lsm(x, f)),
             ("convect", lambda: L.icar_hip_convect(x, f)),
             ("ysu_sfc", lambda: L.icar_hip_ysu_sfc(x)),
             ("lsm_layers", lambda: L.icar_hip_lsm_layers(x, ctypes.byref(nz)))]
    return [(name, call(), L.icar_hip_last_error().decode()) for name, call in calls]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_update_dt_failing_behind_an_early_open_marks_the_context(th_oracle, variant):
    c, dq, opt, d, err = failing(th_oracle, variant)
    assert "context marked failed" in err and "the sub-step was already opened" in err, err
    first = M.run(th_oracle, c, dq, nsteps=1)
    assert d.model_time_seconds == first.t, "the first sub-step completed, the second did not"
    before = downloads(d)
    for name, rc, msg in refused_calls(d):
        assert rc != 0 and REFUSAL in msg and msg.startswith(name + ":"), (name, rc, msg)
    after = downloads(d)
    assert set(before) == set(after) and not [n for n in before if before[n] != after[n]], "a refused call changes no field"
    assert d.model_time_seconds == first.t
    # upload, download and the clock keep working
    qv = (c["water_vapor"] * np.float32(0.5)).astype(np.float32)
    d.set("water_vapor", qv); d.set_dqdt("u", dq["u"])
    assert bits_equal(d.get("water_vapor"), qv) and bits_equal(d.get_dqdt("u"), dq["u"])
    assert refused_calls(d)[1][1] != 0, "uploads do not clear the mark"
    d.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_error_names_its_cause(th_oracle, variant):
    """A NaN wind is carried into the Courant maximum (k_max_courant, icar_amd/csrc/cfl.hip), so the second variant stops with the NaN
    maximum and not, as the reference's MAX and the host model's max_courant would have it, with the dt of the other cells
    (0.0149 s, tests/test_step_loop_model_inputs.py)."""
    err = failing(th_oracle, variant)[3:]
    err[0].close()
    assert VARIANTS[variant]["cause"] in err[1], err[1]


@pytest.mark.parametrize("tile", M.TILES, ids=lambda t: "x".join(map(str, t)))
def test_a_nan_wind_makes_the_courant_maximum_nan(th_oracle, tile):
    """one NaN in u, v or w, in the first and the last lane, row, level and 64-column block: compute_dt names it; an infinite wind is
    no NaN; the finite winds around give the oracle's dt bit for bit"""
    from icar_amd.time_step import compute_dt
    c, dq, opt, (d,) = contexts(th_oracle, tile=tile)
    nx, ny, nz = tile
    want = float(M.cfl_dt(th_oracle, c, c))
    assert compute_dt(d, opt) == want
    spots = {"u": [(0, 0, 0), (ny - 1, nz - 1, nx), (ny // 2, nz // 2, 64 % (nx + 1))],
             "v": [(0, 0, 0), (ny, nz - 1, nx - 1), (1, 1, nx - 3)],
             "w": [(0, 0, 0), (ny - 1, nz - 1, nx - 1), (ny // 2, 1, nx // 2)]}
    for k, where in spots.items():
        for at in where:
            x = c[k].copy(); x[at] = np.nan
            d.set(k, x)
            with pytest.raises(IcarHipError, match="the CFL maximum is NaN"):
                compute_dt(d, opt)
        x = c[k].copy(); x[where[0]] = np.inf
        d.set(k, x)
        with pytest.raises(IcarHipError, match="time step too small"):
            compute_dt(d, opt)
        d.set(k, c[k])
        assert compute_dt(d, opt) == want, k
    d.close()


def fields(d):
    """every field the library hands out"""
    out = {}
    for n in F.NAMES:
        try:
            out[n] = d.get(n)
        except IcarHipError:
            pass
    return out


def test_recovery_equals_a_new_context(th_oracle):
    """Fails on the parent commit: icar_hip_model_time_set cleared the mark and left mp_last_model_time at the time of the failure,
    so the first microphysics call after the recovery ran with mp_dt = 0 (Thompson divides by it)."""
    c, dq, opt, a, _ = failing(th_oracle, "too_large")
    t_fail = a.model_time_seconds
    good, new = contexts(th_oracle, n=2)[3]
    step_n(good, 1, opt, forced=M.FORCED)                                     # the model state at the time of the failure
    assert good.model_time_seconds == t_fail
    state = fields(good)
    for d in (a, new):                                                        # the documented recipe, and the same on a new context
        for n, x in state.items():
            d.set(n, x)
        for k, x in dq.items():
            d.set_dqdt(k, x)
        d.model_time_seconds = t_fail
    dts = [step_n(d, 3, opt, forced=M.FORCED) for d in (a, new)]
    assert dts[0] == dts[1]
    assert_same_state(a, new, "recovered against new")
    r = M.run(th_oracle, c, dq, nsteps=3, t0=t_fail, state={k: state[M.DEVICE_NAME[k]] for k in M.ADV_ORDER + M.WINDS},
              acc0=state["accumulated_precipitation"])
    assert r.n == 3 and dts[0] == r.dts[-1] and a.model_time_seconds == r.t
    for k in M.ADV_ORDER + M.WINDS:
        assert bits_equal(a.get(M.DEVICE_NAME[k]), r.s[k]), k
    assert bits_equal(a.get("exner"), r.diag["exner"]) and bits_equal(a.get("density"), r.diag["density"])
    assert np.array_equal(a.get("accumulated_precipitation"), r.acc) and (r.acc - state["accumulated_precipitation"]).max() > 0
    for d in (a, good, new):
        d.close()


def test_model_time_set_without_the_mark_leaves_the_microphysics_clock(th_oracle):
    """a host that keeps the clock itself sets it after every sub-step: that is no restart"""
    c, dq, opt, (a, b) = contexts(th_oracle, n=2)
    step_n(a, 2, opt, forced=M.FORCED)
    step_n(b, 1, opt, forced=M.FORCED)
    b.model_time_seconds = b.model_time_seconds
    step_n(b, 1, opt, forced=M.FORCED)
    assert_same_state(a, b, "model_time_set between two sub-steps")
    r = M.run(th_oracle, c, dq, nsteps=2)
    assert r.records[1].mp_dt == float(np.float32(r.records[0].dt)) != float(np.float32(r.records[1].dt))
    assert bits_equal(a.get("water_vapor"), r.s["water_vapor"])
    a.close(); b.close()


def test_update_dt_failing_with_nothing_opened_leaves_a_model_state(th_oracle):
    """mp_update_interval > 0 rules the early open out: the failure leaves the fields and the clock of the completed first sub-step
    (the diagnostics aside: those of a sub-step that is not a call's last are unspecified, include/icar_hip.h) and no mark"""
    c, dq = M.case(th_oracle, TILE)
    c, dq, opt, (a, twin) = contexts(th_oracle, M.too_large_tendencies(dq), update_interval=1.0, n=2)
    with pytest.raises(IcarHipError) as e:
        step_n(a, 4, opt, forced=M.FORCED)
    assert "time step too small" in str(e.value) and "marked failed" not in str(e.value), str(e.value)
    step_n(twin, 1, opt, forced=M.FORCED)
    x, y = downloads(a), downloads(twin)
    unspecified = set(DIAGNOSTICS + ["exner"])                                # (the twin's only sub-step is its call's last: it has them all)
    assert set(x) <= set(y) and set(y) - set(x) <= unspecified, sorted(set(x) ^ set(y))
    bad = [n for n in x if x[n] != y[n] and n not in unspecified]
    assert not bad and a.model_time_seconds == twin.model_time_seconds, bad
    for d in (a, twin):                                                       # sane winds and tendencies: it goes on
        d.set("u", c["u"]); d.set_dqdt("u", dq["u"])
        step_n(d, 2, opt, forced=M.FORCED)
    assert_same_state(a, twin, "continued after a failure with nothing opened")
    assert np.isfinite(a.get("potential_temperature")).all()
    a.close(); twin.close()

"""The forcing update on the device (icar_amd/csrc/forcing.hip; include/icar_hip.h, F2) against the CPU restatement
(tests/forcing_oracle.py) and against the compiled reference's vectors in the fixtures directly, bit for bit:
* the six fixtures over both carried forcing steps, entry point by entry point (interpolate_forcing without and with update, the
  forcing's u / v as the in-place smoothing left them, update_delta_fields);
* icar_hip_forcing_step == interpolate_forcing(update), update_winds(update), update_delta_fields made one after the other;
* the same u uploaded once and interpolated twice is smoothed twice, as the restatement's (and the reference's) is;
* every refusal, one out-of-range index in each table among them: the message, and that no field and no table changed."""
import ctypes
import json

import numpy as np
import pytest

import forcing_oracle as FO
from icar_amd import forcing as F
from icar_amd.capi import IcarHipError
from icar_amd.options import options_t

pytestmark = pytest.mark.gpu
_oracle = {}


def oracle(name):
    if name not in _oracle:
        c, z = FO.load_case(name)
        _oracle[name] = (c, z, FO.run_oracle(c))
    return _oracle[name]


def same(got, want, what):
    for k in want:
        if k in got:
            assert FO.bitdiff(got[k], want[k]) == 0, (what, k, FO.bitdiff(got[k], want[k]))


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_fixture_both_steps(name):
    c, z, (data, pre, dq, other, _) = oracle(name)
    d = FO.device_domain(c)
    g_data, g_pre, g_dq, g_lo = FO.device_two_steps(d, c)
    d.close()
    names = FO.forced_of(c)
    assert sorted(g_data) == sorted(names + ["w"]) and sorted(g_dq) == sorted(names + ["w"])
    same(g_data, data, "step 1"); same(g_pre, pre, "interpolate_forcing(update)"); same(g_dq, dq, "update_delta_fields"); same(g_lo, other, "forcing arrays")
    # ... and against the reference's vectors themselves
    held = json.loads(str(z["sha"]))
    for tag, got in (("step1_", g_data), ("step2_pre_", g_pre), ("step2_", g_dq), ("other_", g_lo)):
        for k, v in got.items():
            assert FO.sha(v) == held[tag + k], (tag, k)


def _wind_domain(c):
    """a domain of the case with what update_winds(windtype 0) reads: the jacobians, advection_dz and an unrotated grid"""
    rng = np.random.default_rng(5)
    ny, nz, nx = c["z"].shape
    d = FO.device_domain(c)
    d.set("jacobian_u", rng.uniform(0.9, 1.1, (ny, nz, nx + 1)).astype(FO.f32)); d.set("jacobian_v", rng.uniform(0.9, 1.1, (ny + 1, nz, nx)).astype(FO.f32))
    d.set("jacobian_w", rng.uniform(0.9, 1.1, (ny, nz, nx)).astype(FO.f32)); d.set("jacobian", rng.uniform(0.9, 1.1, (ny, nz, nx)).astype(FO.f32))
    d.set("advection_dz", rng.uniform(50.0, 400.0, (ny, nz, nx)).astype(FO.f32))
    d.set("sintheta", np.zeros((ny, nx), np.float64)); d.set("costheta", np.ones((ny, nx), np.float64))
    d.interpolate_forcing(FO.boundary_of(c, c["lo1"]), update=False)
    d.set("w", c["w"])
    return d


@pytest.mark.parametrize("name", [sorted(FO.CASES)[0], sorted(FO.CASES)[4]])
def test_forcing_step_is_the_three_calls(name):
    from icar_amd.wind import update_winds
    c, z, (data, pre, dq, other, _) = oracle(name)
    names = FO.forced_of(c)
    opt = options_t(); opt.physics.windtype = 0
    a, b = _wind_domain(c), _wind_domain(c)
    F.forcing_step(a, FO.boundary_of(c, c["lo2"]), opt, FO.DT_SECONDS)
    b.interpolate_forcing(FO.boundary_of(c, c["lo2"]), update=True)
    b._winds_initialised = True                                   # update = 1: the forcing step of a run under way
    update_winds(b, opt)
    w_rate = b.get_dqdt("w")
    b.update_delta_fields(FO.DT_SECONDS)
    for n in names + ["w"]:
        ga, gb = a.get_dqdt(n), b.get_dqdt(n)
        assert FO.bitdiff(ga, gb) == 0, (n, FO.bitdiff(ga, gb))
        assert np.isfinite(ga).all()
    # the scalars are untouched by update_winds: the restatement's; w: the restatement's quotient of what balance_uvw left
    for n in names:
        if n not in ("u", "v"):
            assert FO.bitdiff(a.get_dqdt(n), dq[n]) == 0, n
    want = {"w": w_rate.copy()}
    FO.update_delta(want, {"w": c["w"]}, FO.DT_SECONDS, fields=[])
    assert FO.bitdiff(a.get_dqdt("w"), want["w"]) == 0 and float(np.abs(w_rate).max()) > 0
    a.close(); b.close()


def test_same_upload_smoothed_twice():
    c, z, _ = oracle(sorted(FO.CASES)[2])
    ny, nz, nx = c["z"].shape
    d = FO.device_domain(c)
    lo = c["lo1"]["u"].copy()
    F.forcing_upload(d, "u", lo)
    want = []
    for _ in range(2):
        ids = (ctypes.c_int * 1)(d.fid("u"))
        from icar_amd.capi import lib, check
        check(lib().icar_hip_interpolate_forcing(d.ctx, ids, 1, -1, -1, 0), "interpolate_forcing")
        want.append(FO.interp_wind(lo, c["geo_u"], c["nsmooth"], (ny, nz, nx + 1)))
        assert FO.bitdiff(d.get("u"), want[-1]) == 0
        assert FO.bitdiff(F.forcing_download(d, "u", lo.shape), lo) == 0
    assert FO.bitdiff(want[0], want[1]) > 0
    d.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(fn, text):
    with pytest.raises(IcarHipError) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_refusals_leave_everything_as_it_was():
    c, z, (data, pre, dq, other, _) = oracle(sorted(FO.CASES)[3])
    names = FO.forced_of(c)
    ny, nz, nx = c["z"].shape
    d = FO.device_domain(c, configure=False)
    b = FO.boundary_of(c, c["lo1"])
    _refused(lambda: d.interpolate_forcing(b, update=False), "icar_hip_forcing_configure has not been called")
    F.forcing_configure(d, b, c["nsmooth"], domain_z=c["z"])
    d.interpolate_forcing(b, update=False)
    before = {n: d.get(n) for n in names}
    same(before, data, "step 1")

    def still():
        for n in names:
            assert FO.bitdiff(d.get(n), before[n]) == 0, n
        d.interpolate_forcing(FO.boundary_of(c, c["lo1"]), update=False)      # the tables are the ones configured first
        same({n: d.get(n) for n in names if n not in ("u", "v")}, data, "after a refusal")
        for n in ("u", "v"):
            before[n] = d.get(n)

    # one out-of-range index in each table array of each grid
    for g, label in (("geo", "mass"), ("geo_u", "u"), ("geo_v", "v")):
        for key, arr, bad, text in (("x", "x", 0, "geolut%x"), ("x", "x", None, "geolut%x"), ("y", "y", 0, "geolut%y"), ("y", "y", None, "geolut%y"),
                                    ("z", "z", 0, "vert_lut%z"), ("z", "z", None, "vert_lut%z")):
            c2 = dict(c); c2[g] = dict(c[g]); a = c[g][key].copy(); c2[g][key] = a
            top = {"x": c["lo1"]["u"].shape[2], "y": c["lo1"]["u"].shape[0], "z": c["lo1"]["u"].shape[1]}[key]
            a.flat[a.size // 2] = top + 1 if bad is None else bad
            _refused(lambda: F.forcing_configure(d, FO.boundary_of(c2, c["lo1"]), c["nsmooth"], domain_z=c["z"]), f"forcing_configure ({label}): {text}")
        still()
    # shapes, the sub-box, nsmooth, the levels adjust_pressure needs, time_varying_z
    c2 = dict(c); c2["geo_u"] = dict(c["geo_u"]); c2["geo_u"]["i0"] = c["geo_u"]["x"].shape[1] - (nx + 1) + 1      # one past the last offset that fits
    _refused(lambda: F.forcing_configure(d, FO.boundary_of(c2, c["lo1"]), c["nsmooth"], domain_z=c["z"]), "does not lie inside the extended grid")
    c2 = dict(c); c2["geo_v"] = dict(c["geo_v"]); c2["geo_v"]["j0"] = -1
    _refused(lambda: F.forcing_configure(d, FO.boundary_of(c2, c["lo1"]), c["nsmooth"], domain_z=c["z"]), "does not lie inside the extended grid")
    _refused(lambda: F.forcing_configure(d, b, 0, domain_z=c["z"]), "nsmooth = 0")
    _refused(lambda: F.forcing_configure(d, b, c["geo_u"]["x"].shape[1] + 1, domain_z=c["z"]), "is wider than the extended grid")
    _refused(lambda: F.forcing_configure(d, b, c["nsmooth"], domain_z=c["z"], time_varying_z=True), "time_varying_z")
    g2 = F.geo_t(*(c["geo"][k][:, :-1] for k in ("x", "y", "w")), c["geo"]["z"][:, :, :-1], c["geo"]["zw"][:, :, :-1], forcing_shape=c["lo1"]["pressure"].shape)
    _refused(lambda: F.forcing_configure(d, F.boundary_t(g2, b.geo_u, b.geo_v), c["nsmooth"]), "the context's tile is")
    b3 = FO.boundary_of(c, c["lo1"]); b3.geo.nz_f = nz - 1; b3.geo.geo_z = np.ascontiguousarray(c["geo_z"][:, :nz - 1])
    b3.geo.z = np.minimum(b3.geo.z, nz - 1)
    _refused(lambda: F.forcing_configure(d, b3, c["nsmooth"], domain_z=c["z"]), "the reference reads out of bounds")
    still()
    # interpolate_forcing / update_delta_fields
    from icar_amd.capi import lib, check

    def call(fields, pf=-1, tf=-1, update=0):
        ids = (ctypes.c_int * len(fields))(*fields)
        check(lib().icar_hip_interpolate_forcing(d.ctx, ids, len(fields), pf, tf, update), "interpolate_forcing")
    _refused(lambda: call([d.fid("surface_pressure")]), "is 2-D")
    _refused(lambda: call([d.fid("water_vapor"), d.fid("cloud_water")]), "has no forcing data")
    _refused(lambda: call([d.fid("water_vapor"), d.fid("water_vapor")]), "listed twice")
    F.forcing_upload(d, "cloud_water", c["lo1"]["water_vapor"][:, :-1])
    _refused(lambda: call([d.fid("cloud_water")]), "do not have the extents")
    _refused(lambda: F.forcing_upload(d, "surface_pressure", c["lo1"]["water_vapor"]), "is 2-D")
    _refused(lambda: call([d.fid("pressure")], pf=d.fid("pressure"), tf=d.fid("rain_mass")), "potential temperature")
    _refused(lambda: d.update_delta_fields(FO.DT_SECONDS, names), "has no dqdt_3d")
    _refused(lambda: d.update_delta_fields(0.0, names), "positive number of seconds")
    still()
    # without the u / v tables and without the z's: those fields are refused, the others work
    F.forcing_configure(d, F.boundary_t(b.geo), 1)
    _refused(lambda: call([d.fid("u")]), "needs the u / v grids' tables")
    _refused(lambda: call([d.fid("pressure")], pf=d.fid("pressure"), tf=d.fid("potential_temperature")), "needs forcing%geo%z")
    call([d.fid("water_vapor")])
    assert FO.bitdiff(d.get("water_vapor"), data["water_vapor"]) == 0
    d.close()

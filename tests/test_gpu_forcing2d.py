"""The 2-D forced variables on the device (icar_amd/csrc/forcing2d.hip: geo_interp2d, the 2-D delta, the 2-D apply with the
precipitation sum) against the CPU restatement (tests/forcing2d_oracle.py) and against the compiled reference's own vectors
(tests/golden/forcing2d_*.npz), bit for bit in every cell of every array after every stage:
* the six fixtures, entry point by entry point; the fused path (forcing2d_enable + forcing_step) against the separate calls;
* tile widths 3 .. 10, 62 .. 67 and 127 .. 130 with 3 and 5 rows on random valid tables and a 2 x 2 forcing grid;
* a 2 x 2 tiling whose tiles equal the one-image result on every cell of their memory;
* what apply_forcing passes over (a data_2d that is not there; no accumulated precipitation) leaves everything else as it should be;
* every refusal with its text, the state left as it was; a get / set round trip through a new context;
* the 3-D entry points still refuse 2-D fields, the forced ones among them."""
import ctypes

import numpy as np
import pytest

import forcing_oracle as FO
import forcing2d_oracle as F2
from icar_amd import forcing as F
from icar_amd.capi import lib, check, IcarHipError
from icar_amd.options import options_t

pytestmark = pytest.mark.gpu
f32 = np.float32
VARS = F2.VARS


def assert_same(got, want, what=""):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    bad = {k: F2.bitdiff(got[k], want[k]) for k in want if F2.bitdiff(got[k], want[k])}
    assert not bad, (what, bad)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F2.CASES))
def test_fixture_stage_by_stage(name):
    c, z, c3 = F2.load_case(name)
    d = FO.device_domain(c3)
    got = F2.device_chain(d, c)
    d.close()
    assert_same(got, F2.run_oracle(c), "the restatement")
    assert_same(got, {k: z[k] for k in z.files if k not in ("lut_sha", "input_fingerprint")}, "the reference's vectors")


def test_upload_and_download_round_trip():
    c = F2.random_case(1, 9, 4, nxf=5, nyf=3)
    d = F2.device_domain(c)
    for v in VARS:
        F.forcing2d_upload(d, v, c["lo"][1][v])
    for v in VARS:
        assert F2.bitdiff(F.forcing2d_download(d, v, (3, 5)), c["lo"][1][v]) == 0
    with pytest.raises(IcarHipError, match="count does not match the 15 elements uploaded"):
        F.forcing2d_download(d, "sst", (4, 5))
    d.close()


# ---- the fused path -------------------------------------------------------------------------------------------------------------------
def wind_ready(c3):
    """a domain on which icar_hip_forcing_step can run (tests/test_gpu_forcing_step.py, __graft_entry__.smoke_forcing)"""
    rng = np.random.default_rng(11)
    ny, nz, nx = c3["z"].shape
    geom = {"jacobian": (ny, nz, nx), "jacobian_u": (ny, nz, nx + 1), "jacobian_v": (ny + 1, nz, nx), "jacobian_w": (ny, nz, nx)}
    geom = {k: rng.uniform(0.9, 1.1, s).astype(f32) for k, s in geom.items()}
    geom["advection_dz"] = rng.uniform(50.0, 400.0, (ny, nz, nx)).astype(f32)
    d = FO.device_domain(c3)
    for k, v in geom.items():
        d.set(k, v)
    d.set("sintheta", np.zeros((ny, nx))); d.set("costheta", np.ones((ny, nx)))
    d.interpolate_forcing(FO.boundary_of(c3, c3["lo1"]), update=False)
    d.set("w", c3["w"])
    return d


def test_enable_and_forcing_step_equal_the_separate_calls():
    c3 = FO.random_case(3, nx=24, nz=10, ny=12, nxf=7, nzf=6, nyf=9, nsmooth=2, ext=(2, 2, 2, 2))
    rng = np.random.default_rng(12)
    c = {"nx": 24, "ny": 12, "lo": [F2.fields(rng, 9, 7, s) for s in (0.0, 1.5, -1.0)], "acc0": rng.uniform(0.0, 50.0, (12, 24)), "G": c3["geo"]}
    opt = options_t(); opt.physics.windtype = 0
    fused = lambda d, n: F.forcing_step(d, FO.boundary_of(c3, c3["lo2"]), opt, F2.INTERVAL_DT[n - 1])
    a, b = wind_ready(c3), wind_ready(c3)
    got = F2.device_chain(a, c, fused=fused)
    sep = F2.device_chain(b, c)
    want = F2.run_oracle(c)
    assert_same(sep, want, "the separate calls")
    assert_same(got, {k: v for k, v in want.items() if "_pre_" not in k}, "enable + forcing_step")
    # the 3-D part of the step is what it is without the family
    b.interpolate_forcing(FO.boundary_of(c3, c3["lo2"]), update=True)
    assert FO.bitdiff(F.forcing_download(a, "u", c3["lo2"]["u"].shape), F.forcing_download(b, "u", c3["lo2"]["u"].shape)) == 0
    # an enabled variable the step cannot interpolate: refused before the first launch, no rate half-made
    e = wind_ready(c3)
    F.forcing2d_upload(e, "sst", c["lo"][0]["sst"])
    F.forcing2d_enable(e, ["sst", "longwave"])
    with pytest.raises(IcarHipError, match="forcing_step: forced 2-D variable 2 has no forcing data"):
        fused(e, 1)
    with pytest.raises(IcarHipError, match="no dqdt mirror"):
        e.get_dqdt("water_vapor")
    with pytest.raises(IcarHipError, match="has no dqdt_2d on the device"):
        F.forcing2d_get(e, "sst", dqdt=True)
    F.forcing2d_enable(e, [])                                     # n = 0 disables: the step runs again, without the family
    fused(e, 1)
    with pytest.raises(IcarHipError, match="has no dqdt_2d on the device"):
        F.forcing2d_get(e, "sst", dqdt=True)
    for x in (a, b, e):
        x.close()


# ---- tile shapes ----------------------------------------------------------------------------------------------------------------------
WIDTHS = list(range(3, 11)) + list(range(62, 68)) + list(range(127, 131))


@pytest.mark.parametrize("ny", [3, 5])
def test_every_tile_width(ny):
    for nx in WIDTHS:
        c = F2.random_case(100 * ny + nx, nx, ny)
        d = F2.device_domain(c)
        got = F2.device_chain(d, c)
        d.close()
        assert_same(got, F2.run_oracle(c), f"{nx} x {ny}")


def test_two_by_two_tiling_equals_the_one_image_result():
    nxg, nyg, halo = 22, 17, 1
    g = F2.random_case(77, nxg, nyg, nxf=5, nyf=4)
    one = F2.run_oracle(g)
    xs, ys = (0, 11, nxg), (0, 9, nyg)
    for tj in range(2):
        for ti in range(2):
            i_a, i_b = max(0, xs[ti] - halo), min(nxg, xs[ti + 1] + halo)
            j_a, j_b = max(0, ys[tj] - halo), min(nyg, ys[tj + 1] + halo)
            G = {k: np.ascontiguousarray(g["G"][k][j_a:j_b, i_a:i_b] if k in ("x", "y", "w") else g["G"][k][j_a:j_b, :, i_a:i_b]) for k in FO.LUT_KEYS}
            c = {"nx": i_b - i_a, "ny": j_b - j_a, "lo": g["lo"], "acc0": np.ascontiguousarray(g["acc0"][j_a:j_b, i_a:i_b]), "G": G, "luts": G}
            d = F2.device_domain(c)
            got = F2.device_chain(d, c)
            d.close()
            assert_same(got, {k: np.ascontiguousarray(v[j_a:j_b, i_a:i_b]) for k, v in one.items()}, f"tile {ti}, {tj}")


# ---- what apply_forcing passes over ---------------------------------------------------------------------------------------------------
def test_a_variable_without_data_2d_is_passed_over():
    c = F2.random_case(5, 37, 6, nxf=4, nyf=3)
    d = F2.device_domain(c)
    got = F2.device_chain(d, c, no_data=("sst",))
    with pytest.raises(IcarHipError, match="has no data_2d on the device"):
        F.forcing2d_get(d, "sst")
    d.close()
    want = F2.run_oracle(c, no_data=("sst",))
    assert "i2_a1_sst" not in want and "i2_a1_longwave" in want
    assert_same(got, want)


def test_no_accumulated_precipitation_on_the_device_skips_the_sum():
    c = F2.random_case(6, 37, 6, nxf=4, nyf=3)
    d = F2.device_domain(c)
    got = F2.device_chain(d, c, have_acc=False)
    with pytest.raises(IcarHipError):
        d.get("accumulated_precipitation")                        # the apply did not create it either
    d.close()
    assert_same(got, F2.run_oracle(c, have_acc=False))


def test_external_precipitation_not_enabled_leaves_the_sum_alone():
    c = F2.random_case(7, 20, 4, nxf=4, nyf=3)
    d = F2.device_domain(c)
    en = ["longwave", "sst"]
    got = F2.device_chain(d, c, enabled=en)
    d.close()
    want = F2.run_oracle(c, enabled=en)
    assert F2.bitdiff(want["i2_a1_acc"], c["acc0"]) == 0 and F2.bitdiff(want["i2_a1_shortwave"], want["init_shortwave"]) == 0
    assert_same(got, want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def ids(*which):
    return (ctypes.c_int * max(len(which), 1))(*which), len(which)


def raw(name, d, *args):
    check(getattr(lib(), name)(d.ctx, *args), name)


def snapshot(d):
    out = {}
    for v in VARS:
        for what, get in (("lo", lambda: F.forcing2d_download(d, v, (2, 2))), ("data", lambda: F.forcing2d_get(d, v)), ("dqdt", lambda: F.forcing2d_get(d, v, dqdt=True))):
            try:
                out[f"{what}_{v}"] = get().tobytes()
            except IcarHipError:
                out[f"{what}_{v}"] = None
    out["acc"] = d.get("accumulated_precipitation").tobytes()
    return out


def test_refusals_name_the_cause_and_leave_the_state_alone():
    c = F2.random_case(8, 7, 3)
    # before forcing_configure: every entry point that needs the tables
    from icar_amd.domain import domain_t
    from icar_amd.grid import grid_t
    e = domain_t(grid_t().set_grid_dimensions(7, 3, 2, 1, 1), device=0, dx=2000.0)
    lo = c["lo"][0]["sst"]
    i1, n1 = ids(0)
    for name, args in (("icar_hip_forcing2d_upload", (0, lo.ctypes.data_as(ctypes.c_void_p), 2, 2)), ("icar_hip_interpolate_forcing_2d", (i1, n1, 0)),
                       ("icar_hip_update_delta_fields_2d", (i1, n1, 60.0)), ("icar_hip_apply_forcing_2d", (60.0,)), ("icar_hip_forcing2d_enable", (i1, n1))):
        with pytest.raises(IcarHipError, match=name[len("icar_hip_"):] + ": icar_hip_forcing_configure has not been called"):
            raw(name, e, *args)
    e.close()
    # a configured context with sst, shortwave and longwave carried through one interval; external_precipitation never uploaded
    d = F2.device_domain(c)
    three = VARS[:3]
    for v in three:
        F.forcing2d_upload(d, v, c["lo"][0][v])
    d.interpolate_forcing_2d(three, update=False)
    d.interpolate_forcing_2d(three[:2], update=True)              # longwave has no dqdt_2d
    d.set("accumulated_precipitation", c["acc0"])
    F.forcing2d_enable(d, three)
    before = snapshot(d)
    assert before["dqdt_longwave"] is None and before["lo_external_precipitation"] is None and before["dqdt_sst"] is not None
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros((3, 7), f32)
    bad = [
        ("bad forced 2-D variable id 4", "icar_hip_forcing2d_upload", (4, p(lo), 2, 2)),
        ("bad forced 2-D variable id -1", "icar_hip_forcing2d_download", (-1, p(buf), 4)),
        ("bad forced 2-D variable id 7", "icar_hip_interpolate_forcing_2d", (*ids(0, 7), 1)),
        ("bad forced 2-D variable id -1", "icar_hip_update_delta_fields_2d", (*ids(-1), 60.0)),
        ("bad forced 2-D variable id 4", "icar_hip_forcing2d_enable", ids(1, 4)),
        ("bad forced 2-D variable id 9", "icar_hip_forcing2d_get", (9, 0, p(buf))),
        ("bad forced 2-D variable id 9", "icar_hip_forcing2d_set", (9, 1, p(buf))),
        ("what = 2 is neither", "icar_hip_forcing2d_set", (0, 2, p(buf))),
        ("forced 2-D variable 0 is listed twice", "icar_hip_interpolate_forcing_2d", (*ids(0, 1, 0), 1)),
        ("forced 2-D variable 1 is listed twice", "icar_hip_update_delta_fields_2d", (*ids(1, 1), 60.0)),
        ("forced 2-D variable 2 is listed twice", "icar_hip_forcing2d_enable", ids(2, 2)),
        ("bad variable count 5", "icar_hip_forcing2d_enable", ((ctypes.c_int * 5)(0, 1, 2, 3, 0), 5)),
        ("forced 2-D variable 3 has no forcing data", "icar_hip_interpolate_forcing_2d", (*ids(0, 3), 1)),
        ("forced 2-D variable 3 has no forcing data", "icar_hip_forcing2d_download", (3, p(buf), 4)),
        ("the forcing data are 3 x 2, the mass grid's look-up tables were made for 2 x 2", "icar_hip_forcing2d_upload", (0, p(np.zeros((2, 3), f32)), 3, 2)),
        ("forced 2-D variable 2 has no dqdt_2d on the device", "icar_hip_update_delta_fields_2d", (*ids(0, 2), 60.0)),
        ("forced 2-D variable 3 has no dqdt_2d on the device", "icar_hip_forcing2d_get", (3, 1, p(buf))),
    ]
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        bad.append(("dt must be a positive number of seconds", "icar_hip_update_delta_fields_2d", (*ids(0, 1), dt)))
        bad.append(("dt must be a positive number of seconds", "icar_hip_apply_forcing_2d", (dt,)))
    for text, name, args in bad:
        with pytest.raises(IcarHipError, match=name[len("icar_hip_"):] + ": .*" + text.replace("(", r"\(")):
            raw(name, d, *args)
        assert snapshot(d) == before, (name, text)
    # the tables are made again for another forcing grid: the data uploaded for the old one are refused
    G = FO.random_luts(np.random.default_rng(3), 7, 2, 3, 3, 2, 3)
    F.forcing_configure(d, F.boundary_t(F.geo_t(*(G[k] for k in FO.LUT_KEYS), forcing_shape=(3, 2, 3))), 1)
    with pytest.raises(IcarHipError, match="interpolate_forcing_2d: the forcing data of a 2-D variable are 2 x 2, the mass grid's look-up tables were made for 3 x 3"):
        d.interpolate_forcing_2d(["sst"], update=True)
    assert snapshot(d) == before
    d.close()


# ---- restart --------------------------------------------------------------------------------------------------------------------------
def test_get_and_set_carry_a_run_into_a_new_context():
    c = F2.random_case(9, 66, 5, nxf=3, nyf=3)
    want = F2.run_oracle(c)
    a = F2.device_domain(c)
    for v in VARS:
        F.forcing2d_upload(a, v, c["lo"][0][v])
    a.interpolate_forcing_2d(VARS, update=False)
    a.set("accumulated_precipitation", c["acc0"])
    F.forcing2d_enable(a, VARS)
    for v in VARS:
        F.forcing2d_upload(a, v, c["lo"][1][v])
    a.interpolate_forcing_2d(VARS, update=True)
    a.update_delta_fields_2d(VARS, F2.INTERVAL_DT[0])
    a.apply_forcing_2d(F2.APPLY_DT[0][0])
    saved = {(v, q): F.forcing2d_get(a, v, dqdt=q) for v in VARS for q in (False, True)}
    acc = a.get("accumulated_precipitation")
    a.close()
    b = F2.device_domain(c)                                       # the restart: nothing but what was downloaded
    for (v, q), arr in saved.items():
        F.forcing2d_set(b, v, arr, dqdt=q)
    b.set("accumulated_precipitation", acc)
    F.forcing2d_enable(b, VARS)
    got = {}
    for k, dt in list(enumerate(F2.APPLY_DT[0]))[1:]:
        b.apply_forcing_2d(dt)
        got.update({f"i1_a{k}_{v}": F.forcing2d_get(b, v) for v in VARS}); got[f"i1_a{k}_acc"] = b.get("accumulated_precipitation")
    for v in VARS:
        F.forcing2d_upload(b, v, c["lo"][2][v])
    b.interpolate_forcing_2d(VARS, update=True)
    b.update_delta_fields_2d(VARS, F2.INTERVAL_DT[1])
    got.update({f"i2_dq_{v}": F.forcing2d_get(b, v, dqdt=True) for v in VARS})
    for k, dt in enumerate(F2.APPLY_DT[1]):
        b.apply_forcing_2d(dt)
        got.update({f"i2_a{k}_{v}": F.forcing2d_get(b, v) for v in VARS}); got[f"i2_a{k}_acc"] = b.get("accumulated_precipitation")
    b.close()
    assert_same(got, {k: want[k] for k in got})
    assert len(got) == 2 * 5 + 4 + 2 * 5


# ---- the 3-D family ---------------------------------------------------------------------------------------------------------------------
def test_the_3d_entry_points_still_refuse_2d_fields():
    c = F2.random_case(10, 8, 3)
    d = F2.device_domain(c)
    lo3 = np.zeros((2, 2, 2), f32)
    for name in ("sst", "surface_pressure", "shortwave", "longwave"):
        f = d.fid(name)
        one = (ctypes.c_int * 1)(f)
        with pytest.raises(IcarHipError, match=f"forcing_upload: field {f} is 2-D: only 3-D forced fields are built \\(geo_interp2d is not\\)"):
            raw("icar_hip_forcing_upload", d, f, lo3.ctypes.data_as(ctypes.c_void_p), 2, 2, 2)
        with pytest.raises(IcarHipError, match=f"interpolate_forcing: field {f} is 2-D: only 3-D forced fields are built \\(geo_interp2d is not\\)"):
            raw("icar_hip_interpolate_forcing", d, one, 1, -1, -1, 1)
        with pytest.raises(IcarHipError, match=f"update_delta_fields: field {f} is 2-D: the dqdt mirrors are 3-D only"):
            raw("icar_hip_update_delta_fields", d, one, 1, 60.0)
    d.close()

"""The Noah land-surface model on the device against its CPU restatement (tests/support/noah_oracle.c) AND against the vectors of the
compiled reference (tests/golden/noah_*.npz): lsm_init's arrays, the six fixtures over their carried calls (the device carries its own
state from call to call), icar_hip_lsm_noah alone, the upload / download round trips, every refusal with its text and nothing changed,
icar_hip_lsm_init with landsurface = 1 against icar_hip_lsm_configure, and a context that never got the tables.  Every comparison: 0
differing bits."""
import os

import numpy as np
import pytest

import noah_oracle as N
from icar_amd import surface
from icar_amd.capi import IcarHipError, lib
from icar_amd.grid import grid_t
from util import equals_reference_vector, parity_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def tab():
    return N.load_tables()


@pytest.mark.parametrize("name", list(N.CASES))
def test_device_equals_restatement_and_reference_vectors(tab, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = N.make_case(tab, **N.CASES[name])
    assert float(z["input_fingerprint"]) == N.fingerprint(c)
    d = N.device_domain(tab, c)
    A = N.state0(c)
    N.lsm_init(tab, c, A)
    got = N.device_state(d, ["sh2o", "snoalb", "snowh", "canwat", "smois", "tslb", "smstav", "emiss", "albbck", "shdmax", "cqs2", "qgh"])
    for k in ("sh2o", "snoalb", "snowh", "canwat"):
        assert equals_reference_vector(got[k], z["init_" + k]), f"{name}: {k} after lsm_init differs from the compiled reference"
    for k, v in got.items():
        want = A[k] if k in A else np.full(v.shape, {"shdmax": 100.0, "cqs2": 0.01, "qgh": 0.02}[k], np.float32)
        assert N.bitdiff(v, want) == 0, f"{name}: {k} after lsm_init differs from the restatement"
    assert (d.get("land_mask") == c["xland"].astype(np.int32)).all()
    for n in range(N.ncalls(N.CASES[name])):
        N.lsm_noah(tab, c, A, n)
        N.device_forcing(d, c, n)
        surface.lsm_noah(d, float(c["dt"]), *N.tile_of(c))
        got = N.device_state(d)
        for k in N.OUT:
            assert N.bitdiff(got[k], A[k]) == 0, f"{name}, call {n + 1}, {k}: differs from the restatement"
            assert equals_reference_vector(got[k], z[f"call{n + 1}_{k}"]), f"{name}, call {n + 1}, {k}: differs from the compiled reference"
    parity_record("noah", f"fixture/{name}", {k: {"bitdiff_cells": 0} for k in N.OUT})
    d.close()


@pytest.fixture(scope="module")
def case(tab):
    return N.make_case(tab, nx=20, ny=9, seed=41, dt=1200.0, t=[272.0, 276.0], sw=[100, 600], pr=[[0.5, 3.0], [0.3, 2.0]], snow0=0.4, soil_t=273.0)


def test_upload_download_round_trips(tab, case):
    d = N.device_domain(tab, case, init=False)
    rng = np.random.default_rng(5)
    for name in surface.NOAH_ARRAYS:
        shape = (case["ny"], 4, case["nx"]) if surface.NOAH_ID[name] >= surface.NOAH_ID["soil_water_content"] else (case["ny"], case["nx"])
        a = rng.integers(1, 19, shape).astype(np.int32) if name in ("veg_type", "soil_type") else rng.normal(0, 1, shape).astype(np.float32)
        surface.noah_set(d, name, a)
    rng = np.random.default_rng(5)
    for name in surface.NOAH_ARRAYS:                       # ... every array kept its own values: no two of them share memory
        shape = (case["ny"], 4, case["nx"]) if surface.NOAH_ID[name] >= surface.NOAH_ID["soil_water_content"] else (case["ny"], case["nx"])
        a = rng.integers(1, 19, shape).astype(np.int32) if name in ("veg_type", "soil_type") else rng.normal(0, 1, shape).astype(np.float32)
        assert surface.noah_get(d, name).tobytes() == a.tobytes(), name
    with pytest.raises(ValueError):
        surface.noah_set(d, "sh2o", np.zeros((case["ny"], case["nx"]), np.float32))
    d.close()


def snapshot(d):
    out = {k: surface.noah_get(d, k).tobytes() for k in surface.NOAH_ARRAYS}
    out.update({k: d.get(k).tobytes() for k in ("skin_temperature", "sensible_heat", "latent_heat", "qfx", "qsfc", "roughness_z0", "land_mask")})
    return out


def test_refusals_change_nothing(tab, case):
    c = case
    d = N.device_domain(tab, c, init=False)
    N.device_forcing(d, c, 0)
    before = snapshot(d)
    opt = N.options_of(c)
    with pytest.raises(IcarHipError, match="lsm_noah: the scheme is not initialised"):
        surface.lsm_noah(d, 600.0, *N.tile_of(c))
    with pytest.raises(IcarHipError, match="lsm_noah: lsm_dt is positive"):
        surface.lsm_noah(d, 0.0, *N.tile_of(c))
    opt.lsm_options.monthly_vegfrac = True
    with pytest.raises(IcarHipError, match="monthly_vegfrac / monthly_albedo.*not built"):
        surface.noah_init(d, opt)
    opt.lsm_options.monthly_vegfrac = False
    opt.physics.watersurface = 3
    with pytest.raises(IcarHipError, match="kWATER_LAKE.*not built"):
        surface.noah_init(d, opt)
    opt.physics.watersurface = 0
    opt.physics.landsurface = 4
    with pytest.raises(IcarHipError, match="kLSM_NOAHMP.*not built"):
        surface.noah_init(d, opt)
    with pytest.raises(IcarHipError, match=r"kLSM_NOAH\).*not built.*icar_hip_lsm_init"):
        surface.lsm_configure(d, 3)
    assert snapshot(d) == before, "a refusal changed the state"
    for name, key, value in (("veg_type", "ivgtyp", 25), ("veg_type", "ivgtyp", 0), ("soil_type", "isltyp", 20)):   # 25: a USGS category, no row of this data set
        bad = c[key].copy(); bad[2, 3] = value
        surface.noah_set(d, name, bad)
        before = snapshot(d)
        with pytest.raises(IcarHipError, match="names no row of the tables"):
            surface.noah_init(d, N.options_of(c))
        assert snapshot(d) == before, f"the refusal of {name} = {value} changed the state"
        surface.noah_set(d, name, c[key])
    surface.noah_init(d, N.options_of(c))
    before = snapshot(d)
    with pytest.raises(IcarHipError, match="lsm_noah: tile outside memory bounds"):
        surface.lsm_noah(d, 600.0, 0, c["nx"], 1, c["ny"])
    d.configure(N.options_of(c))                                              # the step's tile; the surface slot is as noah_init left it
    with pytest.raises(IcarHipError, match="Noah runs through icar_hip_lsm_noah only"):
        surface.lsm(d, N.options_of(c), 60.0)
    names = ("water_vapor", "temperature", "pressure_interface", "shortwave", "longwave")
    fields = {k: d.get(k).tobytes() for k in names}
    clock = d.model_time_seconds
    for who, f in (("substep", lambda: lib().icar_hip_substep(d.ctx, 10.0, 0)), ("step_n", lambda: lib().icar_hip_step_n(d.ctx, 1, None)),
                   ("step", lambda: lib().icar_hip_step(d.ctx, clock + 100.0, None))):   # refused before diagnostic_update or rad have run
        assert f() != 0
        e = lib().icar_hip_last_error().decode()
        assert e.startswith(who + ": ") and "kLSM_NOAH" in e and "Noah runs through icar_hip_lsm_noah only" in e, e
    assert {k: d.get(k).tobytes() for k in names} == fields and d.model_time_seconds == clock and snapshot(d) == before
    surface.noah_tables(d, tab)                                               # new tables: a new init is needed
    with pytest.raises(IcarHipError, match="not initialised.*or new tables"):
        surface.lsm_noah(d, 600.0, *N.tile_of(c))
    surface.noah_init(d, N.options_of(c))
    before = snapshot(d)
    surface.noah_set(d, "soil_type", c["isltyp"])                             # new categories likewise
    with pytest.raises(IcarHipError, match="not initialised.*again after new veg_type / soil_type"):
        surface.lsm_noah(d, 600.0, *N.tile_of(c))
    assert snapshot(d) == before
    d.close()


def test_lsm_init_s_where_statements(tab):
    """lsm_driver.f90:674-675 and :710 on cells where they do something: a lake and a water category under a land mask that was never
    uploaded (all land), soil temperatures of 0 and soil moistures of 0 under them"""
    c = N.make_case(tab, nx=17, ny=6, seed=81, dt=900.0, t=[274.0], sw=[300], pr=[[0.5, 2.0]], snow0=0.3)
    c["xland"][...] = N.kLC_LAND
    wet = np.zeros(c["xland"].shape, bool); wet[1, 2:5] = True; wet[4, 9] = True
    c["ivgtyp"][~wet & ((c["ivgtyp"] == N.ISWATER) | (c["ivgtyp"] == N.ISLAKE))] = 10
    c["ivgtyp"][wet] = N.ISWATER; c["ivgtyp"][1, 3] = N.ISLAKE; c["isltyp"][wet] = 14
    wet3 = np.repeat(wet[:, None, :], N.NSOIL, axis=1)
    c["tslb0"][wet3] = 0.0; c["smois0"][wet3] = 0.0; c["snow0"][wet] = 0.0; c["snowh0"][wet] = 0.0
    d = N.device_domain(tab, c, land_mask=False)
    A = N.state0(c)
    N.lsm_init(tab, c, A)                                                     # (moves c's xland to water under the two categories)
    assert (c["xland"][wet] == N.kLC_WATER).all() and (c["xland"][~wet] == N.kLC_LAND).all()
    assert (d.get("land_mask") == c["xland"].astype(np.int32)).all()
    assert (A["tslb"][wet3] == 200.0).all() and (A["smois"][wet3] == np.float32(0.0001)).all()
    for k in ("tslb", "smois", "sh2o", "snoalb", "snowh", "canwat"):
        assert N.bitdiff(N.device_get(d, k), A[k]) == 0, k
    N.lsm_noah(tab, c, A, 0)
    N.device_forcing(d, c, 0)
    surface.lsm_noah(d, float(c["dt"]), *N.tile_of(c))
    for k, v in N.device_state(d).items():
        assert N.bitdiff(v, A[k]) == 0, k
    assert (A["diag"][wet] & N.D["WATER"] != 0).all()
    d.close()


def test_missing_uploads_are_named(tab, case):
    from icar_amd.domain import domain_t
    c = case
    d = domain_t(grid_t().set_grid_dimensions(c["nx"], c["ny"], 2, 1, 1), device=0, dx=1000.0)
    with pytest.raises(IcarHipError, match="noah_upload: the Noah tables are not on the device"):
        surface.noah_set(d, "veg_type", c["ivgtyp"])
    with pytest.raises(IcarHipError, match="lsm_init: the Noah tables are not on the device"):
        surface.noah_init(d, N.options_of(c))
    surface.noah_tables(d, tab)
    with pytest.raises(IcarHipError, match="domain%veg_type .* is not on the device"):
        surface.noah_init(d, N.options_of(c))
    d.close()
    d = N.device_domain(tab, c)
    with pytest.raises(IcarHipError, match="CHS .* is not on the device"):
        surface.lsm_noah(d, 600.0, *N.tile_of(c))
    N.device_set(d, "chs", c["forcing"][0]["chs"])
    with pytest.raises(IcarHipError, match="lsm_noah: domain%water_vapor"):
        surface.lsm_noah(d, 600.0, *N.tile_of(c))
    d.close()


def test_lsm_init_with_basic_is_lsm_configure():
    """icar_hip_lsm_init(ctx, 1, ..) leaves the context as icar_hip_lsm_configure(ctx, 1, ..) does: QSFC, and the step state (update interval, the
    two fractions, the layer thickness, the reset gate) through three gated calls of icar_hip_lsm after each"""
    import sfc_oracle as S
    c = S.make_case(nx=22, ny=9, nz=8, seed=11, sh=0.5, lh=0.8, update_interval=200, thick=250.0)
    args = (1, 2, 200, 0.5, 0.8, 250.0)
    out = []
    for use_init in (False, True):
        d = S.device_domain(c)
        for n in range(2):                                                    # a gate that has opened, then other options: both must be forgotten
            S.device_call(d, c, n)
        assert lib().icar_hip_lsm_configure(d.ctx, 1, 0, 50, 1.0, 1.0, 400.0) == 0
        A = S.state(c)
        for k in S.STATE3 + S.STATE2:
            d.set(k, A[k])
        rc = lib().icar_hip_lsm_init(d.ctx, *args, None) if use_init else lib().icar_hip_lsm_configure(d.ctx, *args)
        assert rc == 0
        got = {"qsfc_after_init": d.get("qsfc").tobytes()}
        for n in range(S.CALLS):
            S.device_call(d, c, n)
            got.update({f"{k}_{n}": v.tobytes() for k, v in S.device_state(d).items()})
        got["layers"] = surface.lsm_layers(d, d._sfc_opt)
        out.append(got)
        assert lib().icar_hip_lsm_init(d.ctx, 2, 0, 300, 0.625, 1.0, 400.0, None) != 0 and "Simple LSM not settup" in lib().icar_hip_last_error().decode()
        d.close()
    assert out[0] == out[1]
    A = S.state(c)                                                            # ... and both are what the restatement makes of these options
    for n in range(S.CALLS):
        S.run_oracle(c, A, n)
    for k in S.STATE3 + S.STATE2:
        assert np.ascontiguousarray(A[k]).tobytes() == out[1][f"{k}_{S.CALLS - 1}"], k


def test_a_context_without_the_tables_is_unchanged(tab, case):
    """every Noah entry point refuses a context that never got the tables, and leaves its fields byte for byte as they were"""
    from icar_amd.domain import domain_t
    c = case
    d = domain_t(grid_t().set_grid_dimensions(c["nx"], c["ny"], 2, 1, 1), device=0, dx=1000.0)
    rng = np.random.default_rng(3)
    names = ("water_vapor", "temperature", "pressure_interface", "skin_temperature", "sensible_heat", "latent_heat", "qfx", "qsfc", "roughness_z0", "shortwave",
             "longwave")
    for k in names:
        d.set(k, rng.uniform(0.1, 1.0, d.shape(d.fid(k))).astype(np.float32))
    d.set("land_mask", c["xland"].astype(np.int32))
    before = {k: d.get(k).tobytes() for k in names + ("land_mask",)}
    for f in (lambda: surface.lsm_noah(d, 600.0, *N.tile_of(c)), lambda: surface.noah_init(d, N.options_of(c)), lambda: surface.noah_get(d, "sh2o")):
        with pytest.raises(IcarHipError, match="the Noah tables are not on the device"):
            f()
    assert {k: d.get(k).tobytes() for k in names + ("land_mask",)} == before
    d.close()

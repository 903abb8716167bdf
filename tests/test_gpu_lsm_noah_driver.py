"""The Noah branch of lsm() on the device (icar_amd/csrc/lsm_noah_driver.hip behind icar_hip_lsm_noah_couple) against its CPU restatement
(tests/support/lsm_noah_driver_oracle.c around noah_oracle.c) AND against the vectors of the compiled reference
(tests/golden/lsm_noah_*.npz): the fixtures over their carried calls through surface.lsm with the clock moved between the calls (one call
of each finds the gate shut: every Noah array stays byte for byte and only apply_fluxes acts), every row width around the 64-lane edge, a
sub-range tile, all-water and one-land-cell tiles, every refusal with the state unchanged, a restart through the upload / download pairs,
and a 2 x 2 tiling with a halo.  Every comparison: 0 differing bits."""
import os

import numpy as np
import pytest

import lsm_noah_driver_oracle as LN
import noah_oracle as N
import sfc_oracle as S
from icar_amd import surface
from icar_amd.capi import IcarHipError, lib
from icar_amd.grid import grid_t
from util import equals_reference_vector, parity_record

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = N.OUT + LN.DRV
ALL = KEYS + ["z_atm", "snoalb"]


@pytest.fixture(scope="module")
def tab():
    return N.load_tables()


def device_state(d, keys=KEYS):
    return {k: LN.device_get(d, k) for k in keys}


def same(got, A, keys, what):
    for k in keys:
        assert LN.bitdiff(got[k], A[k]) == 0, f"{what}, {k}: {LN.bitdiff(got[k], A[k])} values differ from the restatement"


class Fluxes:
    """apply_fluxes beside the restatement (tests/sfc_oracle.py): potential_temperature is carried, water_vapor is the call's"""

    def __init__(self, c):
        self.c = dict(LN.atmosphere(c), sh_feedback_fraction=0.625, lh_feedback_fraction=1.0, sfc_layer_thickness=30.0)
        self.th = self.c.pop("potential_temperature").copy()

    def call(self, c, A, n, dt, tile):
        F = c["forcing"][n]
        a = dict(potential_temperature=self.th, water_vapor=np.ascontiguousarray(np.stack([F["qv"], F["qv"]], axis=1)), sensible_heat=A["hfx"],
                 latent_heat=A["lh"])
        S.apply_fluxes(self.c, a, dt, tile=tile, kts=1, kte=2)
        return a


@pytest.mark.parametrize("name", list(LN.CASES))
def test_fixtures_device_equals_restatement_and_reference_vectors(tab, name):
    z = np.load(os.path.join(LN.GOLDEN, name + ".npz"))
    c = LN.make_case(tab, **LN.CASES[name])
    assert float(z["input_fingerprint"]) == LN.fingerprint(c)
    its, ite, jts, jte = LN.tile_of(c)
    t2, t3 = (slice(jts - 1, jte), slice(its - 1, ite)), (slice(jts - 1, jte), slice(None), slice(its - 1, ite))
    d = LN.device_domain(tab, c)
    A = LN.state0(c)
    LN.lsm_init(tab, c, A)
    got = device_state(d, LN.INIT)
    same(got, A, LN.INIT, f"{name} after the coupling")
    for k in LN.INIT:
        assert equals_reference_vector(got[k], z["init_" + k]), f"{name}: {k} after the coupling differs from the compiled reference"
    fl = Fluxes(c)
    closed = 0
    for n in range(len(c["forcing"])):
        before = {k: v.tobytes() for k, v in device_state(d, ALL).items()}
        is_open, _, _ = LN.lsm(tab, c, A, n)
        LN.device_call(d, c, n, dt=30.0 + n)
        got = device_state(d, ALL)
        assert bool(z["gates"][n]) == is_open
        if not is_open:                                                     # only apply_fluxes acted
            closed += 1
            assert {k: v.tobytes() for k, v in got.items()} == before, f"{name}, call {n + 1}: the gate is shut and a Noah array changed"
        same(got, A, KEYS, f"{name}, call {n + 1}")
        for k in KEYS:                                                      # lsm_noah's outputs on its tile, the whole-array statements everywhere
            w = (t3 if got[k].ndim == 3 else t2) if k in N.OUT and k not in LN.WHOLE else Ellipsis
            assert equals_reference_vector(np.ascontiguousarray(got[k][w]), np.ascontiguousarray(z[f"call{n + 1}_{k}"][w])), \
                f"{name}, call {n + 1}, {k}: differs from the compiled reference"
        a = fl.call(c, A, n, 30.0 + n, LN.tile_of(c))
        assert S.bitdiff(d.get("potential_temperature"), a["potential_temperature"]) == 0 and S.bitdiff(d.get("water_vapor"), a["water_vapor"]) == 0
    assert closed == 1
    parity_record("lsm_noah_driver", f"fixture/{name}", {k: {"bitdiff_cells": 0} for k in KEYS})
    d.close()


def small_case(tab, nx, ny=4, seed=50, calls=2, **kw):
    q = dict(nx=nx, ny=ny, seed=seed, dt=900.0, t=[271.0, 277.0, 274.0][:calls], sw=[100, 600, 300][:calls], pr=[[0.5, 3.0], [0.4, 2.0], [0.3, 1.0]][:calls], snow0=0.4,
             soil_t=273.0)
    return LN.make_case(tab, noah=q, seed=seed, closed=99, max_swe=kw.get("max_swe", 30.0))


def run_both(tab, c, grid=None, tile=None):
    d = LN.device_domain(tab, c, grid=grid)
    A = LN.state0(c)
    LN.lsm_init(tab, c, A)
    for n in range(len(c["forcing"])):
        LN.lsm(tab, c, A, n, tile)
        LN.device_call(d, c, n)
    return d, A


@pytest.mark.parametrize("nx", list(range(3, 11)) + list(range(62, 68)) + list(range(127, 131)))
def test_row_widths(tab, nx):
    """ny = 4, nz = 4: the 64-lane edge and the row tail"""
    c = small_case(tab, nx)
    d, A = run_both(tab, c, grid=grid_t().set_grid_dimensions(nx, 4, 4, 1, 1))
    assert (d.nx, d.ny, d.nz) == (nx, 4, 4)
    same(device_state(d, ALL), A, ALL, f"nx = {nx}")
    d.close()


def test_sub_range_tile(tab):
    c = small_case(tab, 70, ny=7, seed=51)
    g = grid_t().set_grid_dimensions(70, 7, 2, 1, 1)
    g.its, g.ite, g.jts, g.jte = 5, 66, 3, 5
    tile = (5, 66, 3, 5)
    d = LN.device_domain(tab, c, grid=g)
    first = device_state(d, ALL)
    A = LN.state0(c)
    LN.lsm_init(tab, c, A)
    for n in range(2):
        LN.lsm(tab, c, A, n, tile)
        LN.device_call(d, c, n)
    got = device_state(d, ALL)
    same(got, A, ALL, "sub-range tile")
    outside = np.ones((7, 70), bool); outside[2:5, 4:66] = False
    for k in ("t2", "q2", "tsk", "hfx", "qsfc", "albedo", "snowh", "canwat"):                  # the tile's statements leave the rest alone
        assert (got[k][outside].view(np.uint32) == first[k][outside].view(np.uint32)).all(), k
        assert (got[k][~outside].view(np.uint32) != first[k][~outside].view(np.uint32)).any(), k
    for k in ("lwup", "smstot", "rib", "chs", "rainbl8"):                                      # the whole-array statements act outside it too
        assert (got[k][outside] != first[k][outside]).any(), k
    d.close()


@pytest.mark.parametrize("land", [0, 1])
def test_all_water_and_one_land_cell_tiles(tab, land):
    c = small_case(tab, 66, ny=5, seed=52 + land)
    keep = np.zeros((5, 66), bool)
    if land:
        keep[2, 64] = True
        c["ivgtyp"][2, 64] = 10; c["isltyp"][2, 64] = 4; c["xland"][2, 64] = N.kLC_LAND
    wet = ~keep
    c["xland"][wet] = N.kLC_WATER; c["ivgtyp"][wet] = N.ISWATER; c["isltyp"][wet] = 14
    c["smois0"][np.repeat(wet[:, None, :], 4, axis=1)] = 1.0; c["snow0"][wet] = 0.0; c["snowh0"][wet] = 0.0
    d, A = run_both(tab, c)
    assert ((A["diag"][1:-1, 1:-1] & N.D["SFLX"]) != 0).sum() == land
    same(device_state(d, ALL), A, ALL, f"{land} land cells")
    d.close()


def snapshot(d, atmosphere=True):
    out = {k: surface.noah_get(d, k).tobytes() for k in surface.NOAH_ARRAYS}
    out.update({k: surface.lsm_get(d, k).tobytes() for k in surface.LSM_ARRAYS})
    out.update({k: d.get(k).tobytes() for k in ("skin_temperature", "sensible_heat", "latent_heat", "qfx", "qsfc", "roughness_z0", "land_mask", "water_vapor",
                                                "temperature") + (("potential_temperature",) if atmosphere else ())})
    return out


def test_refusals_change_nothing(tab):
    c = small_case(tab, 20, ny=6, seed=54)
    opt = LN.options_of(c)
    # before Noah is initialised
    d = N.device_domain(tab, c, init=False)
    LN.device_forcing(d, c, 0)
    before = snapshot(d, False)
    with pytest.raises(IcarHipError, match="lsm_noah_couple: Noah is not initialised"):
        surface.noah_couple(d)
    assert snapshot(d, False) == before
    d.close()
    # each required field missing: the message names it
    for missing in ("z", "terrain", "temperature", "water_vapor", "surface_pressure", "u_10m"):     # (roughness_z0: lsm_noah's own test, test_gpu_noah.py)
        d = N.device_domain(tab, c, init=False)
        for k, a in (("terrain", c["terrain"]), ("z", np.ascontiguousarray(np.stack([c["z1"], c["z1"] + f32(80)], axis=1)))):
            if k != missing:
                d.set(k, a)
        F = c["forcing"][0]
        two = lambda a: np.ascontiguousarray(np.stack([a, a], axis=1))
        for k, a in (("temperature", two(F["t"])), ("water_vapor", two(F["qv"])), ("surface_pressure", F["psfc"]), ("u_10m", F["u10"]), ("v_10m", F["v10"])):
            if k != missing:
                d.set(k, a)
        surface.noah_init(d, opt, fndsnowh=c["fndsnowh"])
        before = {k: surface.noah_get(d, k).tobytes() for k in surface.NOAH_ARRAYS}
        with pytest.raises(IcarHipError, match="lsm_noah_couple: domain%" + ("u_mass" if missing == "u_10m" else missing)):
            surface.noah_couple(d)
        assert {k: surface.noah_get(d, k).tobytes() for k in surface.NOAH_ARRAYS} == before, missing
        with pytest.raises(IcarHipError, match="Noah runs through icar_hip_lsm_noah only"):    # ... and lsm() is as it was
            surface.lsm(d, opt, 30.0)
        d.close()
    # after a coupled run a new lsm_init makes lsm() and the step entry points refuse again, with the texts they always had
    d = LN.device_domain(tab, c)
    LN.device_call(d, c, 0)
    surface.noah_init(d, d._lnd_opt, fndsnowh=c["fndsnowh"])
    before = snapshot(d)
    clock = d.model_time_seconds
    with pytest.raises(IcarHipError, match="Noah runs through icar_hip_lsm_noah only"):
        surface.lsm(d, d._lnd_opt, 30.0)
    for who, f in (("substep", lambda: lib().icar_hip_substep(d.ctx, 10.0, 0)), ("step_n", lambda: lib().icar_hip_step_n(d.ctx, 1, None)),
                   ("step", lambda: lib().icar_hip_step(d.ctx, clock + 100.0, None))):
        assert f() != 0
        e = lib().icar_hip_last_error().decode()
        assert e.startswith(who + ": ") and "kLSM_NOAH" in e and "Noah runs through icar_hip_lsm_noah only" in e, e
    assert snapshot(d) == before and d.model_time_seconds == clock
    surface.noah_couple(d)                                                  # ... and a new coupling runs again
    LN.device_call(d, c, 1)
    surface.noah_tables(d, tab)                                             # new tables: Noah is not initialised any more
    with pytest.raises(IcarHipError, match="Noah runs through icar_hip_lsm_noah only"):
        surface.lsm(d, d._lnd_opt, 30.0)
    with pytest.raises(IcarHipError, match="lsm_noah_couple: Noah is not initialised"):
        surface.noah_couple(d)
    with pytest.raises(IcarHipError, match="lsm_upload: `which` is one of ICAR_LSM_"):
        from icar_amd.capi import check
        check(lib().icar_hip_lsm_upload(d.ctx, 7, np.zeros(4, f32).ctypes.data), "icar_hip_lsm_upload")
    d.close()


def test_restart_through_upload_and_download(tab):
    c = small_case(tab, 30, ny=8, seed=55, calls=3)
    d = LN.device_domain(tab, c)
    for n in range(2):
        LN.device_call(d, c, n)
    noah = {k: surface.noah_get(d, k) for k in surface.NOAH_ARRAYS}
    own = {k: surface.lsm_get(d, k) for k in surface.LSM_ARRAYS}
    fields = {k: d.get(k) for k in ("skin_temperature", "sensible_heat", "latent_heat", "qfx", "qsfc", "roughness_z0", "land_mask", "potential_temperature")}
    LN.device_call(d, c, 2)
    want = snapshot(d)
    d.close()
    r = LN.device_domain(tab, c)                                             # a fresh context: tables, lsm_init, the coupling ...
    for k, a in noah.items():
        if k not in ("veg_type", "soil_type"):                               # (the categories are the case's: new ones would need a new lsm_init)
            surface.noah_set(r, k, a)                                        # ... then everything the first one held
    for k, a in own.items():
        surface.lsm_set(r, k, a)
    for k, a in fields.items():
        r.set(k, a)
    LN.device_call(r, c, 2)
    got = snapshot(r)
    for k in want:
        assert got[k] == want[k], f"{k} after the restart differs from the uninterrupted run"
    r.close()


def test_two_by_two_tiling_with_a_halo(tab):
    c = LN.make_case(tab, **LN.CASES["lsm_noah_a_snowfall_melt_24x12"])
    calls = 3
    d = LN.device_domain(tab, c)
    for n in range(calls):
        LN.device_call(d, c, n)
    one = device_state(d, ALL)
    d.close()
    seen = np.zeros((c["ny"], c["nx"]), int)
    for image in range(1, 5):
        g = grid_t().set_grid_dimensions(c["nx"], c["ny"], 2, 4, image)
        t = LN.device_domain(tab, c, grid=g)
        for n in range(calls):
            LN.device_call(t, c, n)
        got = device_state(t, ALL)
        own = (slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1))
        glob = (slice(g.jts - 1, g.jte), slice(g.its - 1, g.ite))
        seen[glob] += 1
        for k in ALL:
            a, b = (got[k][own], one[k][glob]) if got[k].ndim == 2 else (got[k][own[0], :, own[1]], one[k][glob[0], :, glob[1]])
            assert LN.bitdiff(np.ascontiguousarray(a), np.ascontiguousarray(b)) == 0, f"image {image}, {k}"
        t.close()
    assert (seen[1:-1, 1:-1] == 1).all()

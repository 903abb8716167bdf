"""icar_hip_lsm_noah at the edges of a one-thread-per-cell kernel: every tile width 1 .. 65 with three rows (one lane, a full wave, one
lane of a second block), a sub-range of a larger memory rectangle with the cells outside untouched, tiles that are all water, all land ice
or one land cell, and a 2 x 2 tiling against the one-image result in every owned cell.  Against the CPU restatement, 0 differing bits."""
import numpy as np
import pytest

import noah_oracle as N
from icar_amd import surface
from icar_amd.grid import grid_t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab():
    return N.load_tables()


def started(tab, c):
    """the state after lsm_init and one call, on the host"""
    A = N.state0(c)
    N.lsm_init(tab, c, A)
    N.lsm_noah(tab, c, A, 0)
    return A


def copy(A):
    return {k: v.copy() for k, v in A.items()}


def test_every_tile_width_and_the_cells_outside(tab):
    c = N.make_case(tab, nx=65, ny=5, seed=51, dt=900.0, t=[271.0, 274.0], sw=[200, 700], pr=[[0.5, 3.0], [0.4, 3.0]], snow0=0.5, soil_t=272.5)
    B = started(tab, c)
    full = copy(B)
    N.lsm_noah(tab, c, full, 1)
    d = N.device_domain(tab, c)
    N.device_forcing(d, c, 1)
    for w in range(1, 66):
        tile = (1, w, 2, 4) if w % 2 else (66 - w, 65, 2, 4)
        N.device_put(d, B)
        surface.lsm_noah(d, float(c["dt"]), *tile)
        got = N.device_state(d)
        inside = np.zeros((c["ny"], c["nx"]), bool); inside[tile[2] - 1:tile[3], tile[0] - 1:tile[1]] = True
        for k in N.OUT:
            m = np.broadcast_to(inside[:, None, :], got[k].shape) if got[k].ndim == 3 else inside
            assert N.bitdiff(got[k][m], full[k][m]) == 0, f"width {w}: {k}"
            assert got[k][~m].tobytes() == B[k][~m].tobytes(), f"width {w}: {k} written outside the tile"
    d.close()


@pytest.mark.parametrize("kind", ["water", "land_ice", "one_land_cell"])
def test_uniform_tiles(tab, kind):
    p = dict(nx=13, ny=4, seed=61, dt=1800.0, t=[270.0, 275.0], sw=[0, 500], pr=[[0.5, 2.0], [0.5, 2.0]], snow0=0.5)
    c = N.make_case(tab, **p)
    if kind == "water":
        c["xland"][...] = N.kLC_WATER; c["ivgtyp"][...] = N.ISWATER; c["isltyp"][...] = 14
    elif kind == "land_ice":
        c["xland"][...] = N.kLC_LAND; c["ivgtyp"][...] = N.ISICE; c["isltyp"][...] = 16
    else:
        c["xland"][...] = N.kLC_WATER; c["ivgtyp"][...] = N.ISWATER; c["isltyp"][...] = 14
        c["xland"][2, 7] = N.kLC_LAND; c["ivgtyp"][2, 7] = 10; c["isltyp"][2, 7] = 6
    A = N.state0(c)
    N.lsm_init(tab, c, A)
    d = N.device_domain(tab, c)
    for n in range(2):
        N.lsm_noah(tab, c, A, n)
        N.device_forcing(d, c, n)
        surface.lsm_noah(d, float(c["dt"]), *N.tile_of(c))
        got = N.device_state(d)
        for k in N.OUT:
            assert N.bitdiff(got[k], A[k]) == 0, f"{kind}, call {n + 1}: {k}"
    flag = {"water": "WATER", "land_ice": "LANDICE", "one_land_cell": "SFLX"}[kind]
    assert (A["diag"] & N.D[flag] != 0).sum() == (1 if kind == "one_land_cell" else A["diag"].size)
    d.close()


def test_two_by_two_tiling_equals_one_image(tab):
    c = N.make_case(tab, nx=30, ny=14, seed=71, dt=1200.0, t=[272.0, 277.0], sw=[100, 800], pr=[[0.5, 3.0], [0.3, 2.0]], snow0=0.4, soil_t=273.5)
    A = N.state0(c)
    N.lsm_init(tab, c, A)
    for n in range(2):
        N.lsm_noah(tab, c, A, n)
    owned = 0
    for image in range(1, 5):
        g = grid_t().set_grid_dimensions(c["nx"], c["ny"], 2, 4, image)
        d = N.device_domain(tab, c, grid=g)
        for n in range(2):
            N.device_forcing(d, c, n, d._noah_win)
            surface.lsm_noah(d, float(c["dt"]), g.its, g.ite, g.jts, g.jte)
        got = N.device_state(d)
        rows, cols = slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)
        for k in N.OUT:
            assert N.bitdiff(got[k][rows][..., cols], A[k][g.jts - 1:g.jte][..., g.its - 1:g.ite]) == 0, f"image {image}: {k}"
        owned += (g.jte - g.jts + 1) * (g.ite - g.its + 1)
        d.close()
    assert owned == (c["nx"] - 2) * (c["ny"] - 2)                            # the tiles leave out the domain's outermost ring (grid_obj.f90:228-255)

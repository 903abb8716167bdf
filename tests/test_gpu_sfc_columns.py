"""The surface-flux kernels over their geometry: tile widths of 1 .. 65 columns (a wave edge at 64) and 1 .. 3 rows, level counts
from 2 up, surface layers from one level (nz = 0) to the whole column less one, the refusal where the layer reaches kte, kts > 1, a
sub-range of the tile, and a 2 x 2 tiling against one tile on the owned cells (dz_interface constant per level, so that every image
finds the same nz).  Device against the CPU restatement, 0 differing bits."""
import numpy as np
import pytest

import sfc_oracle as S
from icar_amd import surface
from icar_amd.capi import IcarHipError
from icar_amd.domain import domain_t
from icar_amd.grid import grid_t
from icar_amd.ideal import cut_tile
from util import bits_equal, parity_record

pytestmark = pytest.mark.gpu
FIELDS = S.STATE3 + S.STATE2


def both(c, calls=2, tile=None, parts=None):
    d = S.device_domain(c)
    A = S.state(c)
    for n in range(calls):
        S.device_call(d, c, n, tile=tile, parts=parts)
        S.run_oracle(c, A, n, tile=tile)
    got = S.device_state(d)
    d.close()
    return got, A


@pytest.mark.parametrize("width,rows", [(1, 1), (2, 3), (63, 2), (64, 1), (65, 3)])
def test_tile_widths_and_rows(width, rows):
    c = S.make_case(width + 2, rows + 2, 9, seed=20 + width, update_interval=50)
    got, A = both(c)
    for k in FIELDS:
        assert bits_equal(got[k], A[k]), f"{width} x {rows}, {k}: {S.bitdiff(got[k], A[k])} cells differ"
    parity_record("sfc_columns", f"tile/{width}x{rows}", {k: {"bitdiff_cells": 0} for k in FIELDS})


@pytest.mark.parametrize("nz", [2, 3, 5, 8, 13])
def test_level_counts_and_every_layer_depth(nz):
    """surface layers from one level (nz = 0: sfc_layer_thickness below the first level's dz) to the whole column less one"""
    base = 38.7 * 1.17 ** np.arange(nz)
    depths = set()
    for inside in range(0, nz):                                         # `inside` levels lie below the thickness: the loop runs inside + 1 levels
        thick = float(np.cumsum(base)[inside - 1] + 0.3 * base[inside]) if inside else 0.7 * 0.78 * base[0]
        c = S.make_case(37, 5, nz, seed=30 + nz, thick=thick, update_interval=0)
        assert S.layers(c) == inside, (S.layers(c), inside)
        depths.add(inside)
        got, A = both(c)
        for k in FIELDS:
            assert bits_equal(got[k], A[k]), f"{nz} levels, {inside} inside, {k}: {S.bitdiff(got[k], A[k])} cells differ"
    assert depths == set(range(nz))


def test_a_layer_that_reaches_kte_is_refused_before_anything_is_written():
    c = S.make_case(20, 6, 4, seed=9)                                   # four thin levels: all of them below 400 m
    assert S.layers(c) == 4
    d = S.device_domain(c)
    before = S.device_state(d)
    with pytest.raises(IcarHipError, match="the surface layer reaches kte"):
        surface.apply_fluxes(d, 60.0, 2, 19, 2, 5, 1, 4)
    d.model_time_seconds = 1000.0
    with pytest.raises(IcarHipError, match="reads out of bounds"):
        surface.lsm(d, d._sfc_opt, 60.0)
    after = S.device_state(d)
    for k in S.STATE3:
        assert before[k].tobytes() == after[k].tobytes(), k
    with pytest.raises(ValueError):
        S.apply_fluxes(c, S.state(c), 60.0)
    d.close()


def test_kts_above_the_first_level_and_a_sub_range_of_the_tile():
    """kts = 2: the level search keeps an absolute index, the loop runs kts .. kts+nz, past the layer (the max(0, .) clamp); and a
    tile of one's own inside the memory rectangle"""
    c = S.make_case(44, 9, 14, seed=41, kts=2, update_interval=100)
    got, A = both(c, calls=3)
    for k in FIELDS:
        assert bits_equal(got[k], A[k]), f"kts = 2, {k}: {S.bitdiff(got[k], A[k])} cells differ"
    c = S.make_case(70, 8, 10, seed=42)
    tile = (5, 68, 3, 6)
    got, A = both(c, calls=3, tile=tile)
    for k in FIELDS:
        assert bits_equal(got[k], A[k]), f"sub-tile, {k}: {S.bitdiff(got[k], A[k])} cells differ"
    th0 = c["potential_temperature"]
    outside = np.ones(th0.shape, bool); outside[2:6, :, 4:68] = False
    assert bits_equal(got["potential_temperature"][outside], th0[outside]) and not bits_equal(got["potential_temperature"], th0)


def test_2x2_tiling_equals_tiled_restatement_and_one_tile():
    c = S.make_case(40, 36, 12, seed=7, dz_const=True)
    ny, nz, nx = c["density"].shape
    opts = {k: c[k] for k in ("watersurface", "landsurface", "sfc_layer_thickness", "sh_feedback_fraction", "lh_feedback_fraction", "update_interval", "sfc_dt", "kts")}
    grids = [grid_t().set_grid_dimensions(nx, ny, nz, 4, im) for im in range(1, 5)]
    assert grids[0].ximages == 2 and len({(g.ims, g.jms) for g in grids}) == 4
    one = S.state(c)
    whole = (min(g.its for g in grids), max(g.ite for g in grids), min(g.jts for g in grids), max(g.jte for g in grids))
    for n in range(S.CALLS):
        S.run_oracle(c, one, n, tile=whole)
    owned = np.zeros((ny, nx), bool)
    for im, g in enumerate(grids):
        t = cut_tile(c, g); t.update(opts)
        assert S.layers(t) == S.layers(c)
        d = domain_t(g, device=0, dx=float(c["dx"]), image=im + 1)
        d.load_case(t)
        B = S.state(t)
        for k in S.STATE2:
            d.set(k, B[k])
        d._sfc_opt = S.options_of(t); surface.lsm_init(d, d._sfc_opt); d._sfc_last = -999.0
        tile = (g.its - g.ims + 1, g.ite - g.ims + 1, g.jts - g.jms + 1, g.jte - g.jms + 1)
        for n in range(S.CALLS):
            d.model_time_seconds = S.CLOCK[n]
            surface.diag_10m(d)
            surface.lsm(d, d._sfc_opt, c["sfc_dt"] * (n + 1))           # the tile bounds of the image's own grid
            S.run_oracle(t, B, n, tile=tile)
        got = S.device_state(d)
        for k in FIELDS:
            assert bits_equal(got[k], B[k]), f"image {im + 1}, {k}: {S.bitdiff(got[k], B[k])} cells differ from the tiled restatement"
        js, is_ = slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)
        for k in FIELDS:
            a = got[k][js, :, is_] if got[k].ndim == 3 else got[k][js, is_]
            b = one[k][g.jts - 1:g.jte, :, g.its - 1:g.ite] if one[k].ndim == 3 else one[k][g.jts - 1:g.jte, g.its - 1:g.ite]
            assert bits_equal(a, b), f"image {im + 1}, {k}: the owned cells differ from the one-tile run"
        owned[g.jts - 1:g.jte, g.its - 1:g.ite] = True
        d.close()
    assert owned[1:-1, 1:-1].all()
    parity_record("sfc_columns", "2x2/40x36x12", {k: {"bitdiff_cells": 0} for k in FIELDS})

"""The convection kernels over their geometry: every level count from the smallest accepted one (3) to 66 on 32 x 8 columns, tile
widths of 1 .. 65 columns (a wave edge at 64) x 4 rows x 20 levels, a sub-range its..ite, jts..jte that leaves the rest untouched,
and the refusals: kts = 2, fewer
than 3 levels, more than 129, each before any launch.  Device against the CPU restatement, 0 differing bits."""
import numpy as np
import pytest

import bmj_oracle as B
from icar_amd import convection
from icar_amd.capi import IcarHipError
from icar_amd.domain import domain_t
from icar_amd.grid import grid_t
from util import parity_record

pytestmark = pytest.mark.gpu
RESULTS = ["cldefi", "raincv", "cutop", "cubot", "tend_th", "tend_qv"]
FIELDS = B.STATE3 + B.STATE2
SENT = np.float32(-55.0)


@pytest.mark.parametrize("first", [3, 19, 35, 51])
def test_every_level_count(first):
    deep = shallow = 0
    for nz in range(first, min(first + 16, 67)):
        c = B.make_case(nx=34, ny=10, nz=nz, seed=100 + nz, rh_lo=0.5)          # 32 x 8 owned columns
        d = B.device_domain(c)
        A = B.state(c)
        B.device_call(d, c, 0)
        kind = B.run_oracle(c, A, 0)
        got = B.device_state(d)
        for k in FIELDS:
            assert B.bitdiff(got[k], A[k]) == 0, f"{nz} levels, {k}: {B.bitdiff(got[k], A[k])} cells differ"
        deep += int((kind == B.DEEP).sum()); shallow += int((kind == B.SHALLOW).sum())
        d.close()
    assert deep > 0 and (shallow > 0 or first < 19), (first, deep, shallow)
    parity_record("cu_columns", f"levels/{first}..{min(first + 15, 66)}", {k: {"bitdiff_cells": 0} for k in FIELDS})


def fresh(d, c):
    """the slot's results back to sentinels, CLDEFI to the case's start"""
    ny, nz, nx = c["density"].shape
    for k in ("raincv", "cutop", "cubot"):
        convection.cu_set(d, k, np.full((ny, nx), SENT, np.float32))
    for k in ("tend_th", "tend_qv"):
        convection.cu_set(d, k, np.full((ny, nz, nx), SENT, np.float32))
    convection.cu_set(d, "cldefi", np.full((ny, nx), c["cldefi0"], np.float32))


def expected(c, tile):
    A = B.state(c)
    for k in ("raincv", "cutop", "cubot", "tend_th", "tend_qv"):
        A[k][...] = SENT
    B.drv(c, A, 40.0, tile=tile)
    return A


@pytest.mark.parametrize("widths", [range(1, 23), range(23, 45), range(45, 66)])
def test_tile_widths(widths):
    c = B.make_case(nx=67, ny=6, nz=20, seed=41, rh_lo=0.5)
    d = B.device_domain(c)
    for w in widths:
        tile = (2, 1 + w, 2, 5)                                               # w columns x 4 rows
        fresh(d, c)
        convection.cu_bmj(d, 40.0, *tile)
        A = expected(c, tile)
        for k in RESULTS:
            got = convection.cu_get(d, k)
            assert B.bitdiff(got, A[k]) == 0, f"{w} columns, {k}: {B.bitdiff(got, A[k])} cells differ"
    d.close()
    parity_record("cu_columns", f"widths/{widths[0]}..{widths[-1]}", {k: {"bitdiff_cells": 0} for k in RESULTS})


def test_a_sub_range_leaves_the_rest_untouched():
    c = B.make_case(nx=40, ny=14, nz=20, seed=42, rh_lo=0.5)
    d = B.device_domain(c)
    tile = (7, 29, 4, 9)
    fresh(d, c)
    convection.cu_bmj(d, 40.0, *tile)
    A = expected(c, tile)
    inside = np.zeros((14, 40), bool); inside[3:9, 6:29] = True
    for k in RESULTS:
        got = convection.cu_get(d, k)
        assert B.bitdiff(got, A[k]) == 0, (k, B.bitdiff(got, A[k]))
        if k != "cldefi":
            assert (got[~inside] == SENT).all() if got.ndim == 2 else (got.transpose(0, 2, 1)[~inside] == SENT).all(), f"{k}: written outside the range"
            top = got[:, -1, :][inside] if got.ndim == 3 else None
            assert top is None or (top == SENT).all(), f"{k}: the level kte belongs to nobody (BMJDRV runs on kts..kte-1)"
    assert (convection.cu_get(d, "raincv")[inside] != SENT).all()
    d.close()


def test_refusals_come_before_any_launch():
    # kts = 2: the step is configured with it, the scheme refuses and writes nothing
    c = B.make_case(nx=12, ny=8, nz=10, seed=44)
    g = grid_t().set_grid_dimensions(12, 8, 10, 1, 1)
    g.kts = 2
    d = B.device_domain(c, grid=g)
    fresh(d, c)
    with pytest.raises(IcarHipError, match=r"kts = 2.*DTDT\(1\)"):
        convection.convect(d, d._cu_opt, 40.0)
    with pytest.raises(IcarHipError, match="kts = 2"):
        convection.cu_bmj(d, 40.0, 2, 11, 2, 7)
    assert (convection.cu_get(d, "raincv") == SENT).all() and (convection.cu_get(d, "tend_th") == SENT).all()
    d.close()
    # two levels: one scheme level
    c = B.make_case(nx=12, ny=8, nz=2, seed=45)
    d = B.device_domain(c)
    with pytest.raises(IcarHipError, match=r"at least 3.*PRSMID\(LBOT\+1\)"):
        convection.convect(d, d._cu_opt, 40.0)
    d.close()
    # 131 levels: more than the workspace holds
    c = B.make_case(nx=8, ny=6, nz=131, seed=46)
    d = B.device_domain(c)
    with pytest.raises(IcarHipError, match="at most 129"):
        convection.convect(d, d._cu_opt, 40.0)
    d.close()
    # 129 levels, the most: runs, equal to the restatement
    c = B.make_case(nx=8, ny=6, nz=129, seed=47, rh_lo=0.6)
    d = B.device_domain(c)
    A = B.state(c)
    B.device_call(d, c, 0); B.run_oracle(c, A, 0)
    got = B.device_state(d)
    for k in FIELDS:
        assert B.bitdiff(got[k], A[k]) == 0, (k, B.bitdiff(got[k], A[k]))
    d.close()
    # a field the scheme reads is missing; the tile outside memory
    c = B.make_case(nx=12, ny=8, nz=10, seed=48)
    from util import single_image_domain
    d = single_image_domain({k: v for k, v in c.items() if k != "dz_interface"})
    convection.init_convection(d, B.options_of(c))
    with pytest.raises(IcarHipError, match="dz_interface"):
        convection.cu_bmj(d, 40.0, 2, 11, 2, 7)
    d.set("dz_interface", c["dz_interface"])
    with pytest.raises(IcarHipError, match="outside memory"):
        convection.cu_bmj(d, 40.0, 0, 11, 2, 7)
    d.close()

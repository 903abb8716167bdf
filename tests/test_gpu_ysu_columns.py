"""The YSU kernels over their geometry: every level count from the smallest accepted one (3) to 66, and 129, on 24 x 6 columns; tile
widths of 1 .. 65 columns (a wave edge at 64) at 12 levels; a sub-range its..ite, jts..jte strictly inside the memory that leaves the
rest untouched; a row count that makes the workspace chunking take a short last chunk; and the refusals: kts = 2, one level under the
minimum, one over the cap, a missing roughness_z0 -- each before any launch.  Device against the CPU restatement, 0 differing bits."""
import numpy as np
import pytest

import ysu_oracle as Y
from icar_amd import pbl
from icar_amd.capi import IcarHipError
from icar_amd.grid import grid_t
from util import parity_record, single_image_domain

pytestmark = pytest.mark.gpu
RESULTS = Y.TEND + ["exch_h", "hpbl", "kpbl", "hol"]
FIELDS = Y.STATE3 + ["exch_h"] + Y.OUT2
SENT = np.float32(-55.0)


def one_call(c):
    d = Y.device_domain(c)
    A = Y.state(c)
    Y.device_call(d, c, 0)
    Y.run_oracle(c, A, 0)
    got = Y.device_state(d)
    d.close()
    return got, A


@pytest.mark.parametrize("first", [3, 19, 35, 51, 129])
def test_every_level_count(first):
    mixing = 0
    for nz in range(first, min(first + 16, 67) if first < 129 else 130):
        c = Y.make_case(nx=26, ny=8, nz=nz, seed=100 + nz, lid=min(1200.0 + 300.0 * nz, 14000.0))     # 24 x 6 owned columns
        got, A = one_call(c)
        for k in FIELDS:
            assert Y.bitdiff(got[k], A[k]) == 0, f"{nz} levels, {k}: {Y.bitdiff(got[k], A[k])} cells differ"
        mixing += int((A["kpbl"] > 1).sum())
    assert mixing > 0, first
    parity_record("ysu_columns", f"levels/{first}", {k: {"bitdiff_cells": 0} for k in FIELDS})


def fresh(d, c):
    """ysu's results back to sentinels"""
    ny, nz, nx = c["z"].shape
    for k in RESULTS:
        shape = (ny, nz, nx) if k in pbl.YSU_3D else (ny, nx)
        pbl.ysu_set(d, k, np.full(shape, -55 if k == "kpbl" else SENT, np.int32 if k == "kpbl" else np.float32))


def expected(c, tile):
    A = Y.state(c)
    Y.run_sfc(c, A)
    for k in RESULTS:
        A[k][...] = -55
    Y.run_ysu(c, A, 40.0, tile=tile)
    return A


@pytest.mark.parametrize("widths", [range(1, 23), range(23, 45), range(45, 66)])
def test_tile_widths(widths):
    c = Y.make_case(nx=67, ny=6, nz=12, seed=41, lid=4000.0)
    d = Y.device_domain(c)
    pbl.ysu_sfc(d, d._ysu_opt)
    for w in widths:
        tile = (2, 1 + w, 2, 5)                                               # w columns x 4 rows
        fresh(d, c)
        pbl.ysu(d, 40.0, *tile, 1, 12)
        A = expected(c, tile)
        for k in RESULTS:
            got = pbl.ysu_get(d, k)
            assert Y.bitdiff(got, A[k]) == 0, f"{w} columns, {k}: {Y.bitdiff(got, A[k])} cells differ"
    d.close()
    parity_record("ysu_columns", f"widths/{widths[0]}..{widths[-1]}", {k: {"bitdiff_cells": 0} for k in RESULTS})


def test_a_sub_range_leaves_the_rest_untouched():
    c = Y.make_case(nx=40, ny=14, nz=12, seed=42, lid=4000.0)
    d = Y.device_domain(c)
    pbl.ysu_sfc(d, d._ysu_opt)
    tile = (7, 29, 4, 9)
    fresh(d, c)
    pbl.ysu(d, 40.0, *tile, 1, 12)
    A = expected(c, tile)
    inside = np.zeros((14, 40), bool); inside[3:9, 6:29] = True
    for k in RESULTS:
        got = pbl.ysu_get(d, k)
        assert Y.bitdiff(got, A[k]) == 0, (k, Y.bitdiff(got, A[k]))
        assert (got[~inside] == -55).all() if got.ndim == 2 else (got.transpose(0, 2, 1)[~inside] == -55).all(), f"{k}: written outside the range"
        if got.ndim == 3:
            assert (got[:, -1, :] == -55).all(), f"{k}: the level kte belongs to nobody (ysu runs on kts..kte-1)"
    assert (pbl.ysu_get(d, "hpbl")[inside] != SENT).all() and (pbl.ysu_get(d, "exch_h")[:, -2, :] == SENT).all()
    d.close()


def test_a_short_last_chunk_of_the_workspace():
    """the workspace holds min(nx ny, 2^17) columns; a tile of 410 x 330 = 135300 > 2^17 columns is walked in chunks of 319 rows and a
    last chunk of 11 (3 levels keep it small)"""
    c = Y.make_case(nx=412, ny=332, nz=3, seed=43, lid=1500.0)
    got, A = one_call(c)
    for k in FIELDS:
        assert Y.bitdiff(got[k], A[k]) == 0, (k, Y.bitdiff(got[k], A[k]))
    assert (2 ** 17) // 410 == 319 and 330 % 319 == 11


def test_refusals_come_before_any_launch():
    # kts = 2: the step is configured with it, the scheme refuses and writes nothing
    c = Y.make_case(nx=12, ny=8, nz=10, seed=44)
    g = grid_t().set_grid_dimensions(12, 8, 10, 1, 1)
    g.kts = 2
    d = Y.device_domain(c, grid=g)
    fresh(d, c)
    before = d.get("water_vapor")
    with pytest.raises(IcarHipError, match=r"kts = 2.*level 1 literally"):
        pbl.pbl(d, d._ysu_opt, 40.0)
    with pytest.raises(IcarHipError, match="kts = 2"):
        pbl.ysu(d, 40.0, 2, 11, 2, 7, 2, 10)
    assert (pbl.ysu_get(d, "hpbl") == SENT).all() and (pbl.ysu_get(d, "tend_th") == SENT).all() and d.get("water_vapor").tobytes() == before.tobytes()
    d.close()
    # two levels: one scheme level
    c = Y.make_case(nx=12, ny=8, nz=2, seed=45, lid=800.0)
    d = Y.device_domain(c)
    with pytest.raises(IcarHipError, match=r"at least 3.*za\(i,0\)"):
        pbl.pbl(d, d._ysu_opt, 40.0)
    d.close()
    # 130 levels: one more than the workspace holds
    c = Y.make_case(nx=8, ny=6, nz=130, seed=46, lid=15000.0)
    d = Y.device_domain(c)
    with pytest.raises(IcarHipError, match="at most 129"):
        pbl.pbl(d, d._ysu_opt, 40.0)
    d.close()
    # a field pbl_init reads is missing; then one the scheme reads; the tile outside memory
    c = Y.make_case(nx=12, ny=8, nz=10, seed=48)
    d = single_image_domain({k: v for k, v in c.items() if k not in ("roughness_z0", "dz_interface")})
    with pytest.raises(IcarHipError, match="roughness_z0"):
        pbl.pbl_init(d, Y.options_of(c))
    with pytest.raises(IcarHipError, match="not initialised"):
        pbl.ysu(d, 40.0, 2, 11, 2, 7, 1, 10)
    d.set("roughness_z0", c["roughness_z0"])
    pbl.pbl_init(d, Y.options_of(c))
    with pytest.raises(IcarHipError, match="dz_interface"):
        pbl.ysu(d, 40.0, 2, 11, 2, 7, 1, 10)
    d.set("dz_interface", c["dz_interface"])
    with pytest.raises(IcarHipError, match="outside memory"):
        pbl.ysu(d, 40.0, 0, 11, 2, 7, 1, 10)
    import ctypes
    from icar_amd.capi import lib
    half = np.zeros(48, np.float32)
    assert lib().icar_hip_ysu_upload(d.ctx, 1, half.ctypes.data_as(ctypes.c_void_p), half.size) != 0
    assert "holds 96 values, not 48" in lib().icar_hip_last_error().decode()
    d.close()

"""The NSAS scheme on the device at every level count, every tile width and across workspace chunks, against its CPU restatement
(tests/support/nsas_oracle.c), 0 differing bits:
* every level count from the threshold (3 model levels) to 66, and 129, at 12 x 6 columns;
* tile widths 1..65 at 16 levels over terrain: nsas2d's kbmax / kbm / kmax are the maxima over the columns its..ite of a row
  (cu_nsas.f90:619-632), so the result of a row CHANGES with the width, and equals the restatement at each width;
* a tile of more columns than the workspace holds: the last chunk of rows is a short one."""
import numpy as np
import pytest

import nsas_oracle as N
from icar_amd import convection

pytestmark = pytest.mark.gpu
RES = N.TEND + N.OUT2
LEVELS = list(range(N.MIN_NZ, 67)) + [129]


def _compare(c, d, A, dt, tile, what):
    convection.cu_nsas(d, dt, *tile)
    N.cu_nsas(c, A, dt, tile)
    got = N.device_state(d)
    for k in RES:
        assert N.bitdiff(N.owned(c, got[k], tile), N.owned(c, A[k], tile)) == 0, f"{what}, {k}"


@pytest.mark.parametrize("group", range(4))
def test_every_level_count(group):
    deep = shallow = 0
    for nz in LEVELS[group::4]:
        c = N.make_case(nx=12, ny=6, nz=nz, seed=30 + nz, dx=2000.0 if nz % 2 else 900.0)
        d = N.device_domain(c)
        A = N.state(c)
        _compare(c, d, A, 60.0, (1, 12, 1, 6), f"{nz} levels")
        deep += int((A["diag"] & N.D_DEEP_RAIN != 0).sum()); shallow += int((A["diag"] & N.D_SHALLOW != 0).sum())
        d.close()
    assert deep > 0 and shallow > 0


def test_every_tile_width_over_terrain():
    c = N.make_case(nx=67, ny=4, nz=16, seed=23, terrain=True, dx=4000.0)
    d = N.device_domain(c)
    full = N.state(c)
    _compare(c, d, full, 60.0, (2, 66, 2, 3), "width 65")
    changed = 0
    for w in range(1, 66):
        A = N.state(c)
        _compare(c, d, A, 60.0, (2, 1 + w, 2, 3), f"width {w}")
        changed += any(N.bitdiff(A[k][1:3, ..., 1:1 + w], full[k][1:3, ..., 1:1 + w]) for k in N.TEND)
    assert changed >= 5, "the row's kbmax / kbm / kmax come from the columns its..ite: narrower tiles give other results"
    d.close()


def test_a_short_last_workspace_chunk():
    c = N.make_case(nx=260, ny=130, nz=10, seed=21, dx=3000.0)                # 33 800 columns > 32 768 of the workspace
    d = N.device_domain(c)
    A = N.state(c)
    tile = (2, 259, 2, 129)                                                   # 127 rows of 258 columns fit: 127 + 1
    _compare(c, d, A, 60.0, tile, "two chunks")
    dg = N.owned(c, A["diag"], tile)
    assert (dg[-1] & (N.D_DEEP_RAIN | N.D_SHALLOW) != 0).any(), "the last row, alone in its chunk, convects"
    d.close()

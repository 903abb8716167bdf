"""HIP ra_simple at every column height and tile width: 5 .. 70 levels and 130 on a 66-column tile (the march is unrolled by four
behind its first level: every remainder, and rows of more than one wave), tile widths 1, 2, 63, 64, 65 columns, and sub-ranges
(its > ims + 1, jts = jte, kts .. kte inside the column), all against the CPU restatement, 0 differing bits; fewer than 5 levels
are refused before a launch."""
import numpy as np
import pytest

import ra_oracle as R
from icar_amd import radiation
from icar_amd.capi import IcarHipError
from util import bits_equal, parity_record

pytestmark = pytest.mark.gpu
NY = 5


def run(c, label, tile=None, kts=1, kte=None, calls=2):
    d = R.device_domain(c)
    A = R.state(c)
    for n in range(calls):
        R.device_call(d, c, n, tile=tile, kts=kts, kte=kte)
        R.run_oracle(c, A, n, tile=tile, kts=kts, kte=kte)
        got = R.device_state(d)
        for k in R.OUTPUTS:
            assert bits_equal(got[k], A[k]), f"{label}, call {n + 1}, {k}: {R.bitdiff(got[k], A[k])} of {A[k].size} cells differ"
    d.close()
    assert not np.array_equal(A["potential_temperature"], c["potential_temperature"])
    return A


@pytest.mark.parametrize("nzs", [range(5, 38), range(38, 71), (130,)], ids=lambda r: f"nz{r[0]}-{r[-1]}")
def test_every_level_count(nzs):
    for nz in nzs:
        # a tile of 66 columns; levels of at most 250 m under a 12 km lid (the ideal case's pressure is not a number above 44 km)
        c = R.make_case(68, NY, nz, seed=2000 + nz, D0=40.0 + 0.37 * nz, advance=5000.0, dt=45.0, uniform_dz=min(250.0, 12000.0 / nz))
        assert all(np.isfinite(c[k]).all() for k in R.INPUTS)
        run(c, f"nz = {nz}")
    parity_record("ra_columns", f"nz{nzs[0]}-{nzs[-1]}", {"levels": [int(n) for n in nzs], "bitdiff_cells": 0})


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65])
def test_tile_widths(width):
    c = R.make_case(width + 2, NY, 9, seed=3000 + width, D0=100.4, advance=4000.0)
    run(c, f"{width} columns")
    # ... and the same width away from the memory edge, in the second wave of the row
    c = R.make_case(140, NY, 7, seed=3100 + width, D0=10.6)
    run(c, f"{width} columns from column 66", tile=(66, 65 + width, 2, NY - 1))


@pytest.mark.parametrize("tile,kts,kte", [((5, 17, 3, 9), 1, None), ((2, 29, 7, 7), 1, None), ((9, 9, 2, 19), 1, None), ((3, 28, 3, 18), 3, 9),
                                          ((1, 30, 1, 20), 1, None), ((4, 20, 2, 10), 8, 8)])
def test_sub_ranges(tile, kts, kte):
    """its > ims + 1, a one-row tile, a one-column tile, kts .. kte inside the column, the whole memory extent, a one-level range"""
    c = R.make_case(**R.CASES["ra_simple_d_norunlw_30x20x12"]); c["runlw"] = True
    A = run(c, f"subtile/{tile}/k{kts}-{kte}", tile=tile, kts=kts, kte=kte)
    k0, k1 = kts - 1, (kte or 12)
    outside = np.ones(A["potential_temperature"].shape, bool); outside[tile[2] - 1:tile[3], k0:k1, tile[0] - 1:tile[1]] = False
    assert np.array_equal(A["potential_temperature"][outside], c["potential_temperature"][outside])


def test_fewer_than_five_levels_refused():
    c = R.make_case(12, NY, 7, seed=5)
    d = R.device_domain(c)
    with pytest.raises(IcarHipError, match="ra_simple: at least 5 levels"):
        radiation.ra_simple(d, 60.0, 2, 11, 2, NY - 1, 4, 7)                 # kts + 4 > kme
    for k, v in R.device_state(d).items():
        assert np.array_equal(v, R.state(c)[k]), k
    d.close()

"""The forcing kernels at every geometry edge, device == CPU restatement bit for bit, on look-up tables drawn at random
(tests/forcing_oracle.py:random_case: valid tables that no geometry made, levels below and above the forcing grid among them):
* tile widths 3..65 at 9 levels (a context has at least 3 x 3 columns and 2 levels: narrower tiles cannot be made): below, on and above
  the 64 lanes of a block;
* every model level count 2..66 against 6, 12 and 20 forcing levels; the pressure adjustment runs wherever the forcing has at least the
  model's levels, and is refused where it has fewer;
* nsmooth 1, 2, 3 and 10 on extended grids 3..40 wide (v; u is one wider), the tile's sub-box at an offset; a window wider than the
  extended grid is refused;
* a forcing grid of 2 x 2 columns."""
import numpy as np
import pytest

import forcing_oracle as FO
from icar_amd import forcing as F
from icar_amd.capi import IcarHipError

pytestmark = pytest.mark.gpu


def one_step(c, update, fields=None):
    """interpolate_forcing of step 1 (+ update_delta_fields when update) on the device and in the restatement; returns the differing bits"""
    names = fields or FO.forced_of(c)
    d = FO.device_domain(c)
    lo = {n: c["lo1"][n].copy() for n in FO.FORCED}
    want = {}
    FO.interpolate_forcing(c, lo, want, fields=names)
    d.interpolate_forcing(FO.boundary_of(c, c["lo1"], names), update=update)
    if update:
        data = {n: np.ascontiguousarray(np.random.default_rng(1).standard_normal(want[n].shape), FO.f32) for n in names}
        data["w"], want["w"] = c["w"], c["dqdt_w"].copy()
        for n in names + ["w"]:
            d.set(n, data[n])
        d.set_dqdt("w", c["dqdt_w"])
        d.update_delta_fields(FO.DT_SECONDS)
        FO.update_delta(want, data, FO.DT_SECONDS, fields=names)
        got = {n: d.get_dqdt(n) for n in names + ["w"]}
    else:
        got = {n: d.get(n) for n in names}
    d.close()
    assert all(np.isfinite(v).all() for v in got.values())
    return {n: FO.bitdiff(got[n], want[n]) for n in got}


def test_every_tile_width():
    for nx in range(3, 66):
        c = FO.random_case(nx, nx=nx, nz=9, ny=4, nxf=5, nzf=11, nyf=4, nsmooth=2, ext=(1, 2, 2, 1))
        diff = one_step(c, update=bool(nx % 2))
        assert c["adjust"] and not any(diff.values()), (nx, diff)


@pytest.mark.parametrize("nzf", [6, 12, 20])
def test_every_level_count(nzf):
    adjusted = 0
    for nz in range(2, 67):
        c = FO.random_case(100 * nzf + nz, nx=7, nz=nz, ny=3, nxf=4, nzf=nzf, nyf=3, nsmooth=1, ext=(1, 1, 1, 1))
        diff = one_step(c, update=bool(nz % 2))
        assert c["adjust"] == (nzf >= nz) and ("pressure" in diff) == c["adjust"] and not any(diff.values()), (nz, nzf, diff)
        adjusted += c["adjust"]
        if not c["adjust"]:                                   # fewer forcing levels than the model's: the adjustment is refused
            d = FO.device_domain(c, configure=False)
            b = FO.boundary_of(c, c["lo1"])
            with pytest.raises(IcarHipError, match="the reference reads out of bounds"):
                F.forcing_configure(d, b, 1, domain_z=c["z"])
            d.close()
    assert adjusted == min(nzf, 66) - 1


@pytest.mark.parametrize("nsmooth", [1, 2, 3, 10])
def test_smoothing_windows_on_extended_grids(nsmooth):
    for width in range(3, 41):
        # the extended v grid is `width` wide (u: one more), the tile 3 narrower where there is room, at an offset
        w_, e_ = (1, 2) if width >= 6 else (0, 0)
        nx = width - w_ - e_
        c = FO.random_case(1000 * nsmooth + width, nx=nx, nz=5, ny=4, nxf=5, nzf=6, nyf=4, nsmooth=nsmooth, ext=(w_, e_, 2, 1))
        if nsmooth > width:                                   # smooth_array reads rowmeans(2:windowsize) past the row
            d = FO.device_domain(c, configure=False)
            with pytest.raises(IcarHipError, match="is wider than the extended grid"):
                F.forcing_configure(d, FO.boundary_of(c, c["lo1"]), nsmooth)
            d.close()
            continue
        diff = one_step(c, update=False, fields=["u", "v"])
        assert not any(diff.values()), (nsmooth, width, diff)


def test_two_by_two_forcing_grid():
    c = FO.random_case(77, nx=33, nz=7, ny=5, nxf=2, nzf=8, nyf=2, nsmooth=1, ext=(1, 1, 1, 1))
    for update in (False, True):
        diff = one_step(c, update)
        assert len(diff) >= 5 and not any(diff.values()), diff

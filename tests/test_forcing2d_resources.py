"""The kernels of the 2-D forced variables compile for gfx950 without scratch, without spills and without LDS (CPU only: hipcc
cross-compiles).  The compiler's resource metadata is read, never the instruction stream."""
import os

import pytest

from icar_amd import build as B

KERNELS = ("k_geo_interp2d", "k_delta2d", "k_apply2d")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_forcing2d_kernels_no_scratch_no_spills_no_lds():
    res = B.kernel_resources("forcing2d.hip")
    assert set(res) >= set(KERNELS), sorted(res)
    for k in KERNELS:
        r = res[k]
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0, (k, r)
        # gather / streaming kernels: full occupancy (at most 64 registers)
        assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (k, r)

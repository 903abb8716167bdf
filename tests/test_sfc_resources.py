"""The surface-flux kernels compile for gfx950 without scratch and without spills (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r13_resources_sfc.json, beside the timings (profiles/r13_steps.md)."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_diag_10m", "k_water_simple", "k_apply_fluxes", "k_level_max")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_sfc_kernels_no_scratch_no_spills():
    res = B.kernel_resources("sfc_basic.hip")
    assert set(res) >= set(KERNELS), sorted(res)
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in KERNELS}
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0, (k, r)                  # no LDS, no barrier
        # streaming kernels with one wave per block: they want every wave slot (8 per SIMD need at most 64 registers)
        assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (k, r)
    with open(os.path.join(ROOT, "profiles", "r13_resources_sfc.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")

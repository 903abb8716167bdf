"""The two radiation kernels compile for gfx950 without scratch and without spills (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r12_resources_ra.json, beside the timings measured with it
(profiles/r12_steps.md)."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_ra_kernels_no_scratch_no_spills():
    res = B.kernel_resources("ra_simple.hip")
    assert set(res) >= {"k_ra_simple", "k_ra_latitude"}, sorted(res)
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in ("k_ra_simple", "k_ra_latitude")}
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
    # a streaming kernel with one wave per block: it wants every wave slot (8 per SIMD need at most 64 registers)
    assert rec["k_ra_simple"]["VGPRs"] <= 64 and rec["k_ra_simple"]["Occupancy [waves/SIMD]"] == 8, rec
    with open(os.path.join(ROOT, "profiles", "r12_resources_ra.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")

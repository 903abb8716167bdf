"""The Tiedtke kernels compile for gfx950 without scratch, without spills and without LDS (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r18_resources_tiedtke.json.  The same gates as tests/test_cu_resources.py,
which goes on holding k_cu_zero and k_cu_apply (they now also serve tend%qc and tend%qi)."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMING = ("k_tdk_leveltop",)
COLUMN = ("k_tdk_init", "k_tdk_ascent", "k_tdk_down", "k_tdk_finish")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_tiedtke_kernels_no_scratch_no_spills():
    res = B.kernel_resources("cu_tiedtke.hip")
    assert set(res) >= set(STREAMING + COLUMN), sorted(res)
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in STREAMING + COLUMN}
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0, (k, r)                  # no LDS, no barrier
    for k in STREAMING:
        assert rec[k]["VGPRs"] <= 64 and rec[k]["Occupancy [waves/SIMD]"] == 8, (k, rec[k])
    for k in COLUMN:
        # one thread per column with the column's scalars in registers: at least two waves per SIMD (at most 256 registers)
        assert rec[k]["VGPRs"] <= 256 and rec[k]["Occupancy [waves/SIMD]"] >= 2, (k, rec[k])
    with open(os.path.join(ROOT, "profiles", "r18_resources_tiedtke.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")

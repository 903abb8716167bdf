"""The NSAS kernels compile for gfx950 without scratch, without spills and without LDS (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r19_resources_nsas.json and held to it.  tests/test_cu_resources.py goes
on holding k_cu_zero and k_cu_apply, which also serve this scheme's tend%qc and tend%qi."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMING = ("k_nsas_limits", "k_nsas_finish")
COLUMN = ("k_nsas_deep", "k_nsas_shallow")
RECORD = os.path.join(ROOT, "profiles", "r19_resources_nsas.json")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_nsas_kernels_no_scratch_no_spills():
    res = B.kernel_resources("cu_nsas.hip")
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
    held = json.load(open(RECORD))
    for k in STREAMING + COLUMN:
        assert rec[k]["VGPRs"] <= held[k]["VGPRs"] and rec[k]["Occupancy [waves/SIMD]"] >= held[k]["Occupancy [waves/SIMD]"], (k, rec[k], held[k])

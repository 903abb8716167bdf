"""The forcing kernels compile for gfx950 without scratch, without spills and without LDS (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r20_resources_forcing.json and held to it.  The compiler's resource
metadata is read, never the instruction stream."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_forcing_mass", "k_forcing_mass_novert", "k_adjust_pressure", "k_forcing_box", "k_update_delta")
RECORD = os.path.join(ROOT, "profiles", "r20_resources_forcing.json")
KEEP = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def resources():
    res = B.kernel_resources("forcing.hip")
    return {k: {m: res[k][m] for m in KEEP} for k in KERNELS}


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_forcing_kernels_no_scratch_no_spills_no_lds():
    res = B.kernel_resources("forcing.hip")
    assert set(res) >= set(KERNELS), sorted(res)
    rec = resources()
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0, (k, r)
        # gather / streaming kernels: full occupancy (at most 64 registers)
        assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (k, r)
    held = json.load(open(RECORD))
    for k in KERNELS:
        assert rec[k]["VGPRs"] <= held[k]["VGPRs"] and rec[k]["Occupancy [waves/SIMD]"] >= held[k]["Occupancy [waves/SIMD]"], (k, rec[k], held[k])


if __name__ == "__main__":
    json.dump(resources(), open(RECORD, "w"), indent=1, sort_keys=True)
    print(open(RECORD).read())

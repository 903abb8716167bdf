"""The kernels around k_noah compile for gfx950 without scratch memory and without spills (CPU only: hipcc cross-compiles), and k_noah
itself is what profiles/r21_resources_noah.json records: the pre and post work went into kernels of their own, not into the one that
sits at 256 vector registers."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("k_lsm_noah_couple", "k_lsm_noah_pre", "k_lsm_noah_post")
KEEP = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_driver_kernels_no_scratch_no_spills_no_lds():
    res = B.kernel_resources("lsm_noah_driver.hip")
    assert set(res) >= set(NEW), sorted(res)
    held = json.load(open(os.path.join(ROOT, "profiles", "r22_resources_lsm_noah_driver.json")))
    for k in NEW:
        r = {m: res[k][m] for m in KEEP}
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0 and r["Occupancy [waves/SIMD]"] == 8, (k, r)
        assert r["VGPRs"] <= held[k]["VGPRs"], (k, r, held[k])


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_k_noah_is_what_round_21_recorded():
    res = B.kernel_resources("lsm_noah.hip")
    held = json.load(open(os.path.join(ROOT, "profiles", "r21_resources_noah.json")))
    for k in ("k_noah", "k_noah_init"):
        assert {m: res[k][m] for m in KEEP} == {m: held[k][m] for m in KEEP}, (k, res[k], held[k])

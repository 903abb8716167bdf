"""The Noah kernels compile for gfx950 without scratch memory and without vector-register spills (CPU only: hipcc cross-compiles); what
the register allocator made of them is recorded in profiles/r21_resources_noah.json and held to it.

k_noah holds a cell's whole state in registers: at most 256 vector registers, so that two waves share a SIMD, and nothing in scratch
(the four-layer work arrays are never indexed dynamically; noah_column.h's NOAH_OPAQUE keeps the compiler from turning the select of
ZSOIL(NROOT) into a table in scratch).  The tables are 4.2 KB of LDS per block.  What the compiler does NOT give is a kernel without
scalar-register spills: SFLX's nested divergent control flow needs more exec masks and wave-uniform values than the 102 scalar
registers hold, and 151 of them are spilled -- into lanes of vector registers (v_writelane / v_readlane), not to memory.  The record
holds that number; a build that spills more, or spills to scratch, fails here."""
import json
import os

import pytest

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL = ("k_noah", "k_noah_init")
STREAMING = ("k_noah_mask", "k_noah_floor", "k_noah_fill")
RECORD = os.path.join(ROOT, "profiles", "r21_resources_noah.json")


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc is not present on this host")
def test_noah_kernels_no_scratch_no_vector_spills():
    res = B.kernel_resources("lsm_noah.hip")
    assert set(res) >= set(CELL + STREAMING), sorted(res)
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in CELL + STREAMING}
    held = json.load(open(RECORD))
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["SGPRs Spill"] <= held[k]["SGPRs Spill"], (k, r, held[k])
        assert r["VGPRs"] <= held[k]["VGPRs"] and r["Occupancy [waves/SIMD]"] >= held[k]["Occupancy [waves/SIMD]"], (k, r, held[k])
    for k in STREAMING:
        assert rec[k]["SGPRs Spill"] == 0 and rec[k]["LDS Size [bytes/block]"] == 0 and rec[k]["Occupancy [waves/SIMD]"] == 8, (k, rec[k])
    for k in CELL:
        assert 0 < rec[k]["LDS Size [bytes/block]"] <= 4 * 1047, (k, rec[k])  # the packed tables, once per block (what nothing reads is dropped)
    assert rec["k_noah"]["VGPRs"] <= 256 and rec["k_noah"]["Occupancy [waves/SIMD]"] >= 2, rec["k_noah"]

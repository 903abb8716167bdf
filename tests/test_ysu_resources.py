"""The YSU kernels compile for gfx950 without scratch and without spills (CPU only: hipcc cross-compiles); what the register
allocator made of them is recorded in profiles/r16_resources_ysu.json, beside the timings (profiles/r16_steps.md).

The ceilings.  The three streaming kernels (one thread per cell of the memory, no state): at most 64 VGPRs, which buys all 8 wave
slots of a SIMD.  k_ysu_column (one thread per column, the column's ~50 scalars and its 21 addresses in registers, the level arrays
in the workspace): at most 128 VGPRs, which buys 4 waves per SIMD -- as many as a 512 x 512 tile can supply at all (4096 waves on
1024 SIMDs), so a lower count would buy nothing there."""
import json
import os

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMING = ("k_ysu_init", "k_ysu_sfc", "k_ysu_apply")
COLUMN = ("k_ysu_column",)


def test_ysu_kernels_no_scratch_no_spills():
    assert os.path.exists(B.HIPCC), f"{B.HIPCC}: hipcc is part of the toolchain and is not present"
    res = B.kernel_resources("pbl_ysu.hip")
    mine = sorted(k for k in res if k.startswith("k_ysu_"))
    assert mine == sorted(STREAMING + COLUMN), mine
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in mine}
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 0 and r["AGPRs"] == 0, (k, r)
    for k in STREAMING:
        assert rec[k]["VGPRs"] <= 64 and rec[k]["Occupancy [waves/SIMD]"] == 8, (k, rec[k])
    for k in COLUMN:
        assert rec[k]["VGPRs"] <= 128 and rec[k]["Occupancy [waves/SIMD]"] >= 4, (k, rec[k])
    with open(os.path.join(ROOT, "profiles", "r16_resources_ysu.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")

"""The two boundary-layer kernels compile for gfx950 without scratch and without spills (CPU only: hipcc cross-compiles); what the
register allocator made of them is recorded in profiles/r08_resources_pbl.json, beside the timings measured with it
(profiles/r08_steps.md)."""
import json
import os

from icar_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pbl_kernels_no_scratch_no_spills():
    res = B.kernel_resources("pbl_simple.hip")
    assert set(res) >= {"k_pbl_coef", "k_pbl_diffuse"}, sorted(res)
    keep = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rec = {k: {m: res[k][m] for m in keep} for k in ("k_pbl_coef", "k_pbl_diffuse")}
    for k, r in rec.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
    # two blocks of 1024 threads of k_pbl_diffuse per CU (8 waves per SIMD) need at most 64 registers; the coefficient pass is
    # a streaming kernel that wants every wave slot too
    assert rec["k_pbl_diffuse"]["VGPRs"] <= 64 and rec["k_pbl_coef"]["VGPRs"] <= 64, rec
    rec["note"] = "k_pbl_diffuse uses 48 B of dynamic LDS per thread (two buffers x six scalars), not in the static figure"
    with open(os.path.join(ROOT, "profiles", "r08_resources_pbl.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")

"""The fused MPDATA kernel loads its scalar-independent coefficients as per-face tuples (buffer_load_dwordx3) and per-cell tuples
(buffer_load_dwordx4), not one dword per value (CPU only: hipcc cross-compiles; skipped where there is none).  The kernel is bound
by its loads in flight (profiles/r06_steps.md), so the count of load INSTRUCTIONS is what its time rests on, and it is decided by
the compiler: a compiler update or a change of the source that splits the tuples again shows up here.

Numbers of ROCm 7.2 (hipcc 7.2.26015) for k_mpdata_fused<5, true, true, true>, the variant of the benchmark: 137 buffer loads in
the whole kernel (293 with eleven dword arrays), 68 in the steady loop, which runs two steps of the march per iteration
(34 per step: 16 dwordx3, 5 dwordx4, 13 dword; 81 dword before)."""
import os
import re
import shutil
import subprocess

import pytest
from icar_amd import build as B

METRIC = "_Z14k_mpdata_fusedILi5ELb1ELb1ELb1EE"


@pytest.fixture(scope="module")
def metric_isa(tmp_path_factory):
    if not (os.path.exists(B.HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    out = str(tmp_path_factory.mktemp("isa") / "mpdata.s")
    cmd = [B.HIPCC] + B.FLAGS + B.PER_FILE_FLAGS["mpdata.hip"] + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "mpdata.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    m = re.search(r"^(" + METRIC + r"\w*):", asm, re.M)
    assert m, "the metric variant is not in the code object"
    return asm[m.end(): asm.index(".Lfunc_end", m.end())].splitlines()


def loads(lines):
    return [ln.split()[0] for ln in lines if re.match(r"^\s+buffer_load_", ln)]


def test_coefficients_are_loaded_wide(metric_isa):
    ld = loads(metric_isa)
    assert "buffer_load_dwordx3" in ld and "buffer_load_dwordx4" in ld, sorted(set(ld))
    assert len(ld) <= 150, f"{len(ld)} buffer loads in the kernel (137 with ROCm 7.2; 293 with one dword per value)"


def test_steady_step_issues_at_most_34_loads(metric_isa):
    """the loop with the most loads is the steady one (a pair of steps per iteration): at most 2 x 34 loads"""
    labels = {ln.split(":")[0]: i for i, ln in enumerate(metric_isa) if re.match(r"^\.LBB\w+:", ln)}
    most = []
    for i, ln in enumerate(metric_isa):
        m = re.match(r"^\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            ld = loads(metric_isa[labels[m.group(1)]: i + 1])
            if len(ld) > len(most):
                most = ld
    assert most, "no loop with loads found"
    assert len(most) <= 2 * 34, f"{len(most)} loads in the steady loop of two steps"
    assert most.count("buffer_load_dwordx3") >= 2 * 16 and most.count("buffer_load_dwordx4") >= 2 * 5, sorted(most)

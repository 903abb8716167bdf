"""tests/support/tiedtke_bounds_main.c built as a stand-alone program under the address and undefined-behaviour sanitizers and run:
the restatement of CU_TIEDTKE (icar_amd/csrc/tiedtke_column.h compiled for the host) stays inside its arrays and produces no NaN at
every model level count from 4 to 129, refuses 130, and -- run WITHOUT the refusal -- has a finding at 2 and 3 levels and none at 4:
the smallest count without a finding is the refusal threshold of the library (TDK_MIN_LEVELS + 1 model levels).  CPU hosts only: where
a GPU is present the test skips before it compiles anything (sanitizer programs do not run on GPU machines).  The sanitizer runtimes
are linked statically and the program runs in the environment it is given; nothing is loaded into python."""
import os
import subprocess

import pytest

import tiedtke_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_present():
    try:
        import torch
        if torch.cuda.is_available():
            return True
    except Exception:
        pass
    return os.path.exists("/dev/kfd")


def test_bounds_program_runs_clean_under_the_sanitizers(tmp_path):
    if _gpu_present():
        pytest.skip("a GPU is present: sanitizer programs run on CPU-only hosts, never on a GPU machine")
    exe = str(tmp_path / "tdk_bounds")
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "support", "tiedtke_bounds_main.c"), "-o", exe, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "levels 4..129: no sanitizer finding, no NaN; 130 levels refused"
    ran = [int(l.split()[0]) for l in lines if "convective columns" in l]
    assert ran == list(range(4, 130)) and "130 levels: refused, as it must be" in lines
    assert sum(int(l.split()[2]) for l in lines if "convective columns" in l and int(l.split()[0]) >= 12) > 0, "no convection anywhere"
    # the threshold: without the refusal, the smallest level count that runs without a finding
    clean = []
    for nz in (2, 3, 4, 5):
        q = subprocess.run([exe, str(nz)], capture_output=True, text=True, timeout=120)
        if q.returncode == 0:
            clean.append(nz)
        else:
            assert "Sanitizer" in q.stderr or "runtime error" in q.stderr, q.stderr[-2000:]
    assert clean == [4, 5], clean
    assert T.MIN_NZ == min(clean) == T.MIN_LEVELS() + 1

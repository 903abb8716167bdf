"""tests/support/ysu_bounds_main.c built as a stand-alone program under the address and undefined-behaviour sanitizers and run: the
restatement of the YSU slot (icar_amd/csrc/ysu_column.h compiled for the host) at every level count from 1 to 131 stays inside its
arrays, produces no NaN, and refuses exactly the counts below 3 and above 129.  CPU hosts only: where a GPU is present the test
skips before it compiles anything (sanitizer programs do not run on GPU machines).  The sanitizer runtimes are linked statically and
the program runs in the environment it is given; nothing is loaded into python."""
import os
import subprocess

import pytest

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
    exe = str(tmp_path / "ysu_bounds")
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "support", "ysu_bounds_main.c"), "-o", exe, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "levels 3..129: no sanitizer finding, no NaN; 1, 2, 130, 131 levels refused"
    refused = [int(l.split()[0]) for l in lines if "refused, as it must be" in l]
    ran = [int(l.split()[0]) for l in lines if "largest kpbl" in l]
    assert refused == [1, 2, 130, 131] and ran == list(range(3, 130))

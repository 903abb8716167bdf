"""tests/support/lsm_noah_driver_bounds_main.c -- the restatement of the Noah branch of lsm() around the call under the address and
undefined-behaviour sanitizers, as a stand-alone program (nothing is loaded into python, nothing runs on a GPU): a 3 x 3 and a 65 x 3
memory rectangle, every array an allocation of exactly its extent, tiles touching every edge.  The same program built without the
sanitizers gives the same checksums: the sanitized run computed what the restatement computes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "lsm_noah_driver_bounds_main.c")
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc is not present on this host")


def test_no_finding_on_rectangles_whose_tiles_touch_every_edge(tmp_path):
    out = {}
    for name, flags in (("sanitized", SAN), ("plain", ["-O2", "-ffp-contract=off"])):
        exe = str(tmp_path / name)
        r = subprocess.run(["gcc"] + flags + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-400:], r.stderr[-3000:])
        assert "no finding" in r.stdout and "checksum 3x3" in r.stdout and "checksum 65x3" in r.stdout
        out[name] = [l for l in r.stdout.splitlines() if l.startswith("checksum")]
    assert out["sanitized"] == out["plain"] and len(out["plain"]) == 2

"""tests/support/nsas_bounds_main.c -- the restatement of cu_nsas under the address and undefined-behaviour sanitizers, as a
stand-alone program (nothing is loaded into python, nothing runs on a GPU): every level array of a column is an allocation of exactly
the extent the reference declares, and an index outside it ends the program.
* every scheme level count from NSAS_MIN_LEVELS to 128: no finding, no NaN;
* the smallest count without a finding is the library's threshold: with ONE scheme level nscv2d's unguarded
  xlamue(i,kte) = xlamue(i,km1) (cu_nsas.f90:2456) reads xlamue(i,0); with two there is none (every column leaves at :771 / :2617);
* the workspace filled with two different patterns gives the same checksum, and so does the program built with
  -ftrivial-auto-var-init=zero and =pattern where this gcc has it: no evaluated statement reads what was not written."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "nsas_bounds_main.c")
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc is not present on this host")


def _build(tmp, name, extra=()):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["gcc"] + list(extra) + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    return exe if r.returncode == 0 else None


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nsas_bounds")
    a = _build(tmp, "nan", SAN)
    b = _build(tmp, "zero", SAN + ["-DNSAS_BOUNDS_FILL=0x0u"])
    assert a and b, "the bounds program does not compile"
    return tmp, a, b


def _checksum(out):
    return re.search(r"checksum (\S+)", out).group(1)


def test_threshold_is_two_scheme_levels(programs):
    _, a, _ = programs
    one = subprocess.run([a, "1"], capture_output=True, text=True)
    assert one.returncode != 0 and "FINDING: workspace array 19 " in one.stderr and "level 0 " in one.stderr, one.stderr[-400:]   # NSAS_XLAMB
    two = subprocess.run([a, "2"], capture_output=True, text=True)
    assert two.returncode == 0 and "no finding" in two.stdout, two.stderr[-400:]
    hdr = open(os.path.join(ROOT, "icar_amd", "csrc", "nsas_column.h")).read()
    assert re.search(r"#define NSAS_MIN_LEVELS 2\b", hdr) and re.search(r"NSAS_XLAMB", hdr.split("NSAS_NARR")[0])
    assert hdr.split("NSAS_DEL = 0")[1].split("NSAS_NARR")[0].replace("\n", " ").split(",")[19].strip() == "NSAS_XLAMB"


def test_every_level_count_and_two_workspace_patterns(programs):
    _, a, b = programs
    ra = subprocess.run([a], capture_output=True, text=True)
    rb = subprocess.run([b], capture_output=True, text=True)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr[-600:], rb.stderr[-600:])
    assert "scheme levels 2..128: no finding, no NaN" in ra.stdout
    assert re.search(r"128 scheme levels: [1-9]\d* deep and [1-9]\d* shallow", ra.stdout), "the probe state convects"
    assert _checksum(ra.stdout.splitlines()[-1]) == _checksum(rb.stdout.splitlines()[-1])


def test_uninitialised_locals_change_nothing(programs):
    tmp, _, _ = programs
    z = _build(tmp, "autozero", ["-O1", "-ffp-contract=off", "-ftrivial-auto-var-init=zero"])
    p = _build(tmp, "autopattern", ["-O1", "-ffp-contract=off", "-ftrivial-auto-var-init=pattern"])
    if not z or not p:
        pytest.skip("this gcc has no -ftrivial-auto-var-init")
    outs = [subprocess.run([e, "40"], capture_output=True, text=True) for e in (z, p)]
    assert all(o.returncode == 0 for o in outs)
    assert _checksum(outs[0].stdout) == _checksum(outs[1].stdout)

"""icar_amd/csrc/glibc_flt32_trig.h (the device's sinf / cosf / asinf) compiled for the CPU and compared with the host C library
value by value: tests/glibc_flt32_trig_check.cpp.  In the suite: every 16th REAL(4) bit pattern of each function (268 M arguments
each, seconds); `./check 1` runs all 2^32 (about a minute on 8 cores; 0 mismatches recorded in profiles/r12_steps.md).  The C
library's sincosf is held to its own sinf / cosf on the same arguments: the compiled reference calls all three."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_trig_functions_equal_libm(tmp_path):
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "glibc_flt32_trig_check.cpp"), "-o", exe])
    flags = open("/proc/cpuinfo").read()
    if " fma" not in flags or " avx2" not in flags:
        pytest.skip("this host's glibc selects the non-FMA builds of sinf / cosf")
    out = subprocess.check_output([exe, "16"], text=True, timeout=900)
    seen = {}
    for line in out.splitlines():
        name, n, bad = line.split()[:3]
        seen[name] = (int(n), int(bad))
        assert int(bad) == 0, line
    assert set(seen) == {"sinf", "cosf", "asinf", "sincosf_sin", "sincosf_cos"} and all(n > 1e7 for n, _ in seen.values()), out

"""icar_amd/csrc/glibc_flt32_tan.h (the device's tanf) compiled for the CPU and compared with the host C library value by
value: tests/glibc_flt32_tanf_check.cpp.  In the suite: every 16th REAL(4) bit pattern (268 M arguments, seconds); `./check 1`
runs all 2^32 (half a minute on 8 cores; 0 mismatches recorded in profiles/r17_steps.md).  tanf has one build in the C library
(no FMA variant), so the comparison holds on any x86-64 host of that glibc."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_tanf_equals_libm(tmp_path):
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "glibc_flt32_tanf_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe, "16"], text=True, timeout=900)
    name, n, bad = out.split()[:3]
    assert name == "tanf" and int(n) == 1 << 28, out
    assert int(bad) == 0, out

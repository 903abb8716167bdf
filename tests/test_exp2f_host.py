"""gf_exp2f of icar_amd/csrc/glibc_flt32.h (the device's exp2f: LLVM turns the Noah scheme's 2.0 ** x into exp2) compiled for the CPU
and compared with the host C library value by value: tests/support/exp2f_check.cpp, every 16th REAL(4) bit pattern (268 M
arguments); `./check 1` runs all 2^32."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_exp2f_equals_libm(tmp_path):
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "support", "exp2f_check.cpp"), "-o", exe])
    flags = open("/proc/cpuinfo").read()
    if " fma" not in flags or " avx2" not in flags:
        pytest.skip("this host's glibc selects the non-FMA build of exp2f")
    name, n, bad = subprocess.check_output([exe, "16"], text=True, timeout=900).split()[:3]
    assert name == "exp2f" and int(n) > 1e8 and int(bad) == 0

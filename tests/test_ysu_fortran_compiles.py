"""The Fortran bindings of the YSU entry points, type-checked: tests/support/ysu_glue.f90 calls hip_pbl_init, hip_ysu_sfc, hip_ysu,
hip_ysu_upload, hip_ysu_download (2-D and 3-D actual arguments through the assumed-rank dummies) and hip_ysu_download_kpbl as
INTEGRATION.md's "YSU" paragraph shows them, and flang must accept it against icar_amd/fortran/icar_hip_mod.f90; a call with a wrong
kind must be rejected.  CPU only, compile only."""
import os
import re
import subprocess

import pytest

from icar_amd.build import FLANG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")
GLUE = os.path.join(ROOT, "tests", "support", "ysu_glue.f90")


@pytest.fixture(scope="module")
def moddir(tmp_path_factory):
    assert os.path.exists(FLANG), f"{FLANG}: flang is part of the toolchain (icar_amd.build.FLANG) and is not present"
    d = str(tmp_path_factory.mktemp("ysu_mod"))
    subprocess.check_call([FLANG, "-O0", "-c", MOD, "-o", os.path.join(d, "icar_hip_mod.o"), "-module-dir", d])
    return d


def check(moddir, path):
    return subprocess.run([FLANG, "-fsyntax-only", "-I" + moddir, "-module-dir", moddir, path], capture_output=True, text=True)


def test_the_caller_compiles(moddir):
    r = check(moddir, GLUE)
    assert r.returncode == 0, r.stderr[-3000:]


def test_every_call_integration_shows_is_in_the_caller():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    para = doc[doc.index("**YSU.**"):doc.index("**Radiation.**")]
    shown = set(re.findall(r"call (hip_[a-z_0-9]+)\(", para))
    assert shown >= {"hip_pbl_init", "hip_ysu_upload", "hip_pbl", "hip_ysu_sfc", "hip_ysu", "hip_ysu_download", "hip_ysu_download_kpbl"}, shown
    glue = open(GLUE).read()
    for name in shown:
        assert re.search(r"call " + name + r"\(", glue), f"{name}: shown in INTEGRATION.md, not compiled by tests/support/ysu_glue.f90"


def test_a_wrong_binding_is_rejected(moddir, tmp_path):
    bad = open(GLUE).read().replace("integer, intent(inout), target, contiguous :: kpbl(:,:)", "real(8), intent(inout), target, contiguous :: kpbl(:,:)")
    assert bad != open(GLUE).read()
    p = tmp_path / "bad.f90"
    p.write_text(bad)
    assert check(moddir, str(p)).returncode != 0, "a REAL(8) kpbl must not pass hip_ysu_download_kpbl"

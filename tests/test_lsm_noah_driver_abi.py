"""The entry points of the Noah branch of lsm() at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in
icar_amd/capi.py and the Fortran module, exported by the library; enum icar_hip_lsm_array agrees between the three and leaves the
existing enums alone; a null context is refused with the entry point's name; the header cites the Fortran lines each replaces; the
Fortran binding compiles together with the host-side glue tests/support/integration_glue_lsm_noah.f90."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from icar_amd import capi, surface
from icar_amd.build import FLANG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_lsm_noah_couple", "icar_hip_lsm_upload", "icar_hip_lsm_download"]


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        from icar_amd import build
        build.build()
    return capi.lib()


def test_entry_points_declared_bound_exported_and_documented():
    text = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    L = _lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for s in ENTRY:
        assert re.search(r"\bint\s+" + s + r"\s*\(\s*icar_hip_ctx\s*\*\s*ctx\b", hdr), f"{s} is not declared with the context first"
        assert s in capi.SYMBOLS and hasattr(L, s) and s in exported, s
        assert f'bind(C, name="{s}")' in mod and ("hip_" + s[len("icar_hip_"):]) in mod, f"{s}: no Fortran binding"
    doc = text.split("---- L3:")[1].split("enum icar_hip_lsm_array")[0]
    for lines in (":566", ":583-587", ":592-596", ":602-603", ":610-611", ":992", ":993-997", ":1016-1023", ":1028", ":244-265", ":1144-1147", ":1181-1187",
                  "atm_utilities.f90:523-560", ":1207", ":1208", ":1210-1278", ":1280", ":1282-1286", ":1289", ":1290", ":1524-1527", ":299-359", ":337-352",
                  ":119-129", ":1550-1552", "time_step.f90:491", ":269-297"):
        assert lines in doc, lines
    for word in ("icar_hip_lsm_noah_couple", "icar_hip_lsm_upload", "exchange_term = 1", "NOT built", "rain_fraction", "associated(T2bare)"):
        assert word in doc, word


def test_enum_values_agree_and_the_existing_ones_stay():
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    for n, name in enumerate(surface.LSM_ARRAYS):
        assert ids["ICAR_LSM_" + name.upper()] == n == surface.LSM_ID[name], name
        assert re.search(r"\bICAR_LSM_" + name.upper() + r"=" + str(n) + r"\b", mod), name
    assert ids["ICAR_LSM_N"] == len(surface.LSM_ARRAYS) == 7 and re.search(r"ICAR_LSM_N=7\b", mod)
    assert surface.LSM_ARRAYS == ["temperature_2m", "humidity_2m", "longwave_up", "rainbl", "z_atm", "lnz_atm_term", "base_exchange_term"]
    assert ids["ICAR_NOAH_N"] == 42 and ids["ICAR_N_FIELD_SLOTS"] == 63 and ids["ICAR_LSM_NOAH"] == 3 and len(surface.NOAH_ARRAYS) == 42


def test_a_null_context_is_refused_with_the_entry_point_s_name():
    L = _lib()
    err = lambda: L.icar_hip_last_error().decode()
    buf = (ctypes.c_float * 4)()
    assert L.icar_hip_lsm_noah_couple(None) != 0 and err().startswith("lsm_noah_couple: ") and "null argument" in err()
    assert L.icar_hip_lsm_upload(None, 0, buf) != 0 and err().startswith("lsm_upload: ") and "null argument" in err()
    assert L.icar_hip_lsm_download(None, 0, buf) != 0 and err().startswith("lsm_download: ") and "null argument" in err()


def test_python_mirror():
    for n in ("noah_couple", "lsm_set", "lsm_get", "lsm"):
        assert callable(getattr(surface, n))
    import inspect
    assert list(inspect.signature(surface.lsm).parameters) == ["domain", "options", "dt"]


def test_the_sources_say_what_is_not_built():
    cell = open(os.path.join(ROOT, "icar_amd", "csrc", "lsm_noah_driver_cell.h")).read()
    for word in ("exchange_term = 1", "F2_formula", "temperature_2m_bare", "rain_fraction", "rain_bucket"):
        assert word in cell, word
    from icar_amd import build as B
    assert "lsm_noah_driver.hip" in B.SOURCES


@pytest.mark.skipif(not (os.path.exists(FLANG) or shutil.which(FLANG)), reason="flang is not present on this host")
def test_fortran_binding_and_the_integration_glue_compile(tmp_path):
    mod = os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")
    run = lambda path: subprocess.run([FLANG, "-fsyntax-only", "-I" + str(tmp_path), "-module-dir", str(tmp_path), path], capture_output=True, text=True)
    r = run(mod)
    assert r.returncode == 0, r.stderr[-3000:]
    r = run(os.path.join(ROOT, "tests", "support", "integration_glue_lsm_noah.f90"))
    assert r.returncode == 0, r.stderr[-3000:]

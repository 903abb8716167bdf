"""The YSU entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the Fortran
module, exported by the library; the refusals that need no context; the Python mirror of pbl_driver.f90's YSU branches.  (A context
needs a device: the refusals of kts = 2, of too few and too many levels and of a missing roughness_z0 are GPU tests,
tests/test_gpu_ysu_columns.py.)"""
import ctypes
import os
import re
import subprocess

from icar_amd import capi, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_pbl_init", "icar_hip_ysu_sfc", "icar_hip_ysu", "icar_hip_ysu_upload", "icar_hip_ysu_download"]
ARRAYS = ["GROUND_SURF_TEMPERATURE", "HPBL", "KPBL", "EXCH_H", "PSIM", "PSIH", "REGIME", "RI", "WINDSPD", "HOL", "ZOL", "GZ1OZ0", "Z_ATM", "TEND_TH",
          "TEND_QV", "TEND_QC", "TEND_QI", "TEND_U", "TEND_V"]


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        from icar_amd import build
        build.build()
    return capi.lib()


def test_entry_points_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icar_hip.h")).read(), flags=re.S)
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    L = _lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for s in ENTRY:
        assert re.search(r"\bint\s+" + s + r"\s*\(\s*icar_hip_ctx\s*\*\s*ctx\b", hdr), f"{s} is not declared with the context first in include/icar_hip.h"
        assert s in capi.SYMBOLS and hasattr(L, s) and s in exported, s
        assert f'bind(C, name="{s}")' in mod and ("hip_" + s[len("icar_hip_"):]) in mod, f"{s}: no Fortran binding"


def test_enum_values_agree():
    from icar_amd import pbl
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert ids["ICAR_PBL_YSU"] == 3 == K.kPBL_YSU and "ICAR_PBL_YSU = 3" in mod
    for n, name in enumerate(ARRAYS):
        assert ids["ICAR_YSU_" + name] == n == pbl.YSU_NAMES[name.lower()], name
        assert re.search(r"\bICAR_YSU_" + name + r"=" + str(n) + r"\b", mod), name
    assert ids["ICAR_YSU_N"] == len(ARRAYS) == len(pbl.YSU_NAMES)
    # no new field ids
    assert ids["ICAR_N_FIELDS"] == 47 and ids["ICAR_N_FIELD_IDS"] == 52 and ids["ICAR_N_FIELD_SLOTS"] == 63


def test_refusals_without_a_device():
    L = _lib()
    err = lambda: L.icar_hip_last_error().decode()
    assert L.icar_hip_pbl_init(None, 3) != 0 and err().startswith("pbl_init: ") and "null ctx" in err()
    assert L.icar_hip_pbl_init(None, 2) != 0 and "null ctx" in err()
    assert L.icar_hip_pbl_init(None, 7) != 0 and "boundarylayer is 0, 1" in err() and "kPBL_YSU" in err()
    assert L.icar_hip_pbl_init(None, -1) != 0 and err().startswith("pbl_init: ")
    assert L.icar_hip_ysu_sfc(None) != 0 and err().startswith("ysu_sfc: ")
    assert L.icar_hip_ysu(None, ctypes.c_float(10.0), 1, 1, 1, 1, 1, 3) != 0 and err().startswith("ysu: ")
    buf = (ctypes.c_float * 4)()
    assert L.icar_hip_ysu_upload(None, 0, buf, 4) != 0 and err().startswith("ysu_upload: ")
    assert L.icar_hip_ysu_download(None, 0, buf, 4) != 0 and err().startswith("ysu_download: ")
    # the option setter keeps refusing YSU, and says where it is selected
    assert L.icar_hip_pbl_configure(None, 3) != 0
    assert "YSU" in err() and "not built" in err() and "icar_hip_pbl_init(ctx, 3)" in err()


def test_python_mirror():
    from icar_amd import pbl
    from icar_amd.options import options_t
    for n in ("pbl_var_request", "pbl_init", "pbl", "ysu_sfc", "ysu", "ysu_get", "ysu_set", "pbl_finalize"):
        assert callable(getattr(pbl, n))
    opt = options_t()
    opt.physics.boundarylayer = K.kPBL_YSU
    pbl.pbl_var_request(opt)
    # pbl_driver.f90:76-102: 35 names are allocated and written to restart files, four scalars are advected
    assert len(pbl.YSU_VARS) == 35 and opt.vars_to_advect == {"potential_temperature": 1, "water_vapor": 1, "cloud_ice": 1, "cloud_water": 1}
    for n in ("hpbl", "kpbl", "coeff_heat_exchange_3d", "roughness_z0", "ustar", "ground_surf_temperature", "tend_qv_pbl", "land_mask"):
        assert n in opt.vars_to_allocate, n

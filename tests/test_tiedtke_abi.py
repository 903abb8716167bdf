"""The Tiedtke entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the
Fortran module, exported by the library; the refusals that need no context; the Python mirror of cu_driver.f90's Tiedtke branches.
(A context needs a device: the refusals of kts = 2 and of too few and too many levels are GPU tests, tests/test_gpu_tiedtke.py.)"""
import ctypes
import os
import re
import subprocess

from icar_amd import capi, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_cu_init", "icar_hip_cu_tiedtke", "icar_hip_tiedtke_upload", "icar_hip_tiedtke_download"]
ARRAYS = ["TEND_QC", "TEND_QI", "PRATEC", "KTYPE"]


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
    from icar_amd import convection
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert ids["ICAR_CU_TIEDTKE"] == 1 == K.kCU_TIEDTKE == convection.kCU_TIEDTKE and "ICAR_CU_TIEDTKE = 1" in mod
    for n, name in enumerate(ARRAYS):
        assert ids["ICAR_TIEDTKE_" + name] == n == convection.TIEDTKE_NAMES[name.lower()], name
        assert re.search(r"\bICAR_TIEDTKE_" + name + r"=" + str(n) + r"\b", mod), name
    assert ids["ICAR_TIEDTKE_N"] == len(ARRAYS) == convection.TIEDTKE_N
    # the slot's own enum and the field ids are what they were
    assert ids["ICAR_CU_N"] == 7 and ids["ICAR_N_FIELDS"] == 47 and ids["ICAR_N_FIELD_IDS"] == 52 and ids["ICAR_N_FIELD_SLOTS"] == 63


def test_refusals_without_a_device():
    L = _lib()
    cf = ctypes.c_float
    err = lambda: L.icar_hip_last_error().decode()
    znu = (ctypes.c_float * 8)(*[1.0 - (k + 0.5) / 8 for k in range(8)])
    init = lambda cu, st=-9999.0, tf=1.0, z=znu: L.icar_hip_cu_init(None, cu, cf(st), cf(tf), cf(-1), cf(-1), cf(-1), cf(-1), z)
    assert init(1) != 0 and err().startswith("cu_init: ") and "null ctx" in err()
    assert init(1, z=None) != 0 and "znu" in err()
    assert init(1, st=20.0) != 0 and "stochastic_cu" in err()
    assert init(1, tf=float("nan")) != 0 and "NaN" in err()
    # 0 and 5 do what icar_hip_cu_configure does, and so do the schemes that are not built; the messages name this entry point
    assert init(5, z=None) != 0 and err().startswith("cu_init: ") and "null ctx" in err()
    assert init(0, z=None) != 0 and "null ctx" in err()
    assert init(4) != 0 and "kCU_NSAS" in err() and "not built" in err()
    assert init(2) != 0 and "kCU_SIMPLE" in err()
    assert init(3) != 0 and "kCU_KAINFR" in err()
    assert init(7) != 0 and err().startswith("cu_init: ")
    assert L.icar_hip_cu_tiedtke(None, cf(10.0), 1, 1, 1, 1) != 0 and err().startswith("cu_tiedtke: ")
    buf = (ctypes.c_float * 4)()
    assert L.icar_hip_tiedtke_upload(None, 0, buf) != 0 and err().startswith("tiedtke_upload: ")
    assert L.icar_hip_tiedtke_download(None, 0, buf) != 0 and err().startswith("tiedtke_download: ")
    # the option setter keeps refusing Tiedtke, and says where it is selected
    assert L.icar_hip_cu_configure(None, 1, cf(-9999.0), cf(1), cf(-1), cf(-1), cf(-1), cf(-1)) != 0
    assert "kCU_TIEDTKE" in err() and "not built" in err() and "icar_hip_cu_init" in err()


def test_python_mirror():
    from icar_amd import convection
    from icar_amd.options import options_t
    for n in ("cu_var_request", "init_convection", "convect", "cu_init", "cu_tiedtke", "tiedtke_get", "tiedtke_set"):
        assert callable(getattr(convection, n))
    opt = options_t()
    opt.physics.convection = K.kCU_TIEDTKE
    convection.cu_var_request(opt)
    # cu_driver.f90:43-50: the Tiedtke list has the two moisture tendencies and znu on top of what every scheme asks for
    for n in ("tend_qv_pbl", "tend_qv_adv", "znu", "tend_qc", "tend_qi", "w", "land_mask"):
        assert n in opt.vars_to_allocate, n
    assert opt.vars_to_advect == {"potential_temperature": 1, "water_vapor": 1}

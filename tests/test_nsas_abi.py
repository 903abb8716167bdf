"""The NSAS entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the Fortran
module, exported by the library; the refusals that need no context; the Python mirror of cu_driver.f90's NSAS branches.  The
earlier entry points keep refusing convection = 4 and name icar_hip_convection_init.
(A context needs a device: the refusals of kts = 2 and of too few and too many levels are GPU tests, tests/test_gpu_nsas.py.)"""
import ctypes
import os
import re
import subprocess

from icar_amd import capi, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_convection_init", "icar_hip_cu_nsas", "icar_hip_nsas_upload", "icar_hip_nsas_download"]
ARRAYS = ["TEND_QC", "TEND_QI", "PRATEC", "HBOT", "HTOP", "HPBL"]


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
    # each entry cites the reference's lines
    doc = open(os.path.join(ROOT, "include", "icar_hip.h")).read().split("---- C3:")[1].split("enum { ICAR_CU_NSAS")[0]
    for s in ENTRY[:3]:
        assert re.search(re.escape(s) + r" ==? ?.*?\(.*?:\d+", doc, flags=re.S) or s in doc, s
    assert "cu_driver.f90:97-253" in doc and ":363-417" in doc and "cu_nsas.f90:619-632" in doc


def test_enum_values_agree():
    from icar_amd import convection
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert ids["ICAR_CU_NSAS"] == 4 == K.kCU_NSAS == convection.kCU_NSAS and "ICAR_CU_NSAS = 4" in mod
    for n, name in enumerate(ARRAYS):
        assert ids["ICAR_NSAS_" + name] == n == convection.NSAS_NAMES[name.lower()], name
        assert re.search(r"\bICAR_NSAS_" + name + r"=" + str(n) + r"\b", mod), name
    assert ids["ICAR_NSAS_N"] == len(ARRAYS) == convection.NSAS_N and re.search(r"ICAR_NSAS_N=6\b", mod)
    # the other enums and the field ids are what they were
    assert ids["ICAR_CU_N"] == 7 and ids["ICAR_TIEDTKE_N"] == 4 and ids["ICAR_YSU_N"] == 19
    assert ids["ICAR_N_FIELDS"] == 47 and ids["ICAR_N_FIELD_IDS"] == 52 and ids["ICAR_N_FIELD_SLOTS"] == 63


def test_refusals_without_a_device():
    L = _lib()
    cf = ctypes.c_float
    err = lambda: L.icar_hip_last_error().decode()
    znu = (ctypes.c_float * 8)(*[1.0 - (k + 0.5) / 8 for k in range(8)])
    init = lambda cu, st=-9999.0, tf=1.0, z=znu, dx=2000.0: L.icar_hip_convection_init(None, cu, cf(st), cf(tf), cf(-1), cf(-1), cf(-1), cf(-1), z, cf(dx))
    assert init(4) != 0 and err().startswith("convection_init: ") and "null ctx" in err()
    for dx in (0.0, -5.0, float("nan"), float("inf")):                       # the values are looked at before the context
        assert init(4, dx=dx) != 0 and "dx" in err() and "null ctx" not in err(), dx
    assert init(4, st=20.0) != 0 and "stochastic_cu" in err()
    assert init(4, tf=float("nan")) != 0 and "NaN" in err()
    # 0, 5 and 1 do what icar_hip_cu_init does (dx ignored); the messages name this entry point
    assert init(5, z=None, dx=0.0) != 0 and err().startswith("convection_init: ") and "null ctx" in err()
    assert init(0, z=None, dx=-1.0) != 0 and "null ctx" in err()
    assert init(1, dx=0.0) != 0 and err().startswith("convection_init: ") and "null ctx" in err()
    assert init(1, z=None) != 0 and "znu" in err()
    assert init(2) != 0 and "kCU_SIMPLE" in err()
    assert init(3) != 0 and "kCU_KAINFR" in err()
    assert init(7) != 0
    assert L.icar_hip_cu_nsas(None, cf(10.0), 1, 1, 1, 1) != 0 and err().startswith("cu_nsas: ")
    buf = (ctypes.c_float * 4)()
    assert L.icar_hip_nsas_upload(None, 0, buf) != 0 and err().startswith("nsas_upload: ")
    assert L.icar_hip_nsas_download(None, 0, buf) != 0 and err().startswith("nsas_download: ")


def test_the_earlier_entry_points_keep_refusing_nsas_and_name_the_new_one():
    L = _lib()
    cf = ctypes.c_float
    err = lambda: L.icar_hip_last_error().decode()
    znu = (ctypes.c_float * 8)(*[0.5] * 8)
    assert L.icar_hip_cu_configure(None, 4, cf(-9999.0), cf(1), cf(-1), cf(-1), cf(-1), cf(-1)) != 0
    assert "kCU_NSAS" in err() and "not built" in err() and "icar_hip_convection_init" in err() and err().startswith("cu_configure: ")
    assert L.icar_hip_cu_init(None, 4, cf(-9999.0), cf(1), cf(-1), cf(-1), cf(-1), cf(-1), znu) != 0
    assert "kCU_NSAS" in err() and "not built" in err() and "icar_hip_convection_init" in err() and err().startswith("cu_init: ")


def test_python_mirror():
    from icar_amd import convection
    from icar_amd.options import options_t
    for n in ("cu_var_request", "init_convection", "convect", "convection_init", "cu_nsas", "nsas_get", "nsas_set"):
        assert callable(getattr(convection, n))
    opt = options_t()
    opt.physics.convection = K.kCU_NSAS
    convection.cu_var_request(opt)
    # cu_driver.f90:59-73: the NSAS list has hpbl on top of what every scheme asks for, and writes it to restart files
    for n in ("hpbl", "tend_qc", "tend_qi", "tend_u", "tend_v", "w", "land_mask", "sensible_heat", "latent_heat"):
        assert n in opt.vars_to_allocate, n
    assert "znu" not in opt.vars_to_allocate and "kpbl" not in opt.vars_to_allocate
    assert "hpbl" in opt.vars_for_restart
    assert opt.vars_to_advect == {"potential_temperature": 1, "water_vapor": 1}

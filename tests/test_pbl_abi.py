"""The boundary-layer entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py
and the Fortran module, exported by the library; the argument checks that need no context.  (A context needs a device: the
refusals of a one-level call and of more than 1024 levels are GPU tests, tests/test_gpu_pbl_columns.py.)"""
import os
import re
import subprocess

from icar_amd import capi, _fields as F, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_pbl_simple", "icar_hip_pbl_configure", "icar_hip_pbl"]


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
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/icar_hip.h"
        assert s in capi.SYMBOLS and hasattr(L, s) and s in exported, s
        assert f'bind(C, name="{s}")' in mod and ("hip_" + s[len("icar_hip_"):]) in mod, f"{s}: no Fortran binding"


def test_field_ids_and_element_sizes():
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert ids["ICAR_F_TERRAIN"] == 45 == F.TERRAIN and ids["ICAR_F_LAND_MASK"] == 46 == F.LAND_MASK
    assert ids["ICAR_N_FIELDS"] == 47 == F.N_FIELDS and ids["ICAR_PBL_SIMPLE"] == 2 == K.kPBL_SIMPLE
    assert F.NAMES["terrain"] == 45 and F.NAMES["land_mask"] == 46 and (K.kLC_LAND, K.kLC_WATER) == (1, 2)
    L = _lib()
    assert L.icar_hip_field_elem_size(45) == 4 and L.icar_hip_field_elem_size(46) == 4       # REAL(4) and INTEGER(4)
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    assert "ICAR_F_TERRAIN=45" in mod and "ICAR_F_LAND_MASK=46" in mod


def test_pbl_configure_refuses_ysu_without_a_device():
    L = _lib()
    assert L.icar_hip_pbl_configure(None, 3) != 0
    msg = L.icar_hip_last_error().decode()
    assert "YSU" in msg and "not built" in msg, msg
    assert L.icar_hip_pbl_configure(None, 7) != 0 and "boundarylayer is 0, 1" in L.icar_hip_last_error().decode()
    assert L.icar_hip_pbl_configure(None, 2) != 0 and "null ctx" in L.icar_hip_last_error().decode()


def test_python_mirror_names():
    from icar_amd import pbl
    from icar_amd.options import options_t
    for n in ("pbl_var_request", "pbl_init", "pbl", "pbl_finalize"):
        assert callable(getattr(pbl, n))
    opt = options_t()
    assert opt.physics.boundarylayer == 0
    opt.physics.boundarylayer = K.kPBL_SIMPLE
    pbl.pbl_var_request(opt)
    assert not opt.vars_to_allocate and not opt.vars_to_advect, "pbl_driver.f90:62 tests landsurface: nothing is requested"
    opt.physics.landsurface = 2
    pbl.pbl_var_request(opt)
    assert opt.vars_to_advect == {"potential_temperature": 1, "water_vapor": 1} and "land_mask" in opt.vars_to_allocate

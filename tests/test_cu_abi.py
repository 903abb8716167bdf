"""The convection entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the
Fortran module, exported by the library; the ICAR_CU_* names in the header, Python and Fortran (the slot's arrays have no field
id: ICAR_N_FIELD_SLOTS stays 63); every refusal that needs no context, with its message; the level-count refusals held in the source
in front of every launch; the Python mirror's names and the reference's defaults."""
import os
import re
import subprocess

from icar_amd import capi, _fields as F, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_cu_configure", "icar_hip_cu_bmj", "icar_hip_convect", "icar_hip_cu_reset", "icar_hip_cu_upload", "icar_hip_cu_download"]
ARRAYS = ["CLDEFI", "ACC_CONV_PCP", "RAINCV", "CUTOP", "CUBOT", "TEND_TH", "TEND_QV"]
NO_STOCH = -9999.0


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
    for s in ENTRY + ["icar_hip_cu_tables"]:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/icar_hip.h"
        assert s in capi.SYMBOLS and hasattr(L, s) and s in exported, s
    for s in ENTRY:
        assert f'bind(C, name="{s}")' in mod and ("hip_" + s[len("icar_hip_"):]) in mod, f"{s}: no Fortran binding"


def test_cu_array_names_in_header_python_and_fortran():
    from icar_amd import convection as C
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    for n, name in enumerate(ARRAYS):
        assert ids["ICAR_CU_" + name] == n == getattr(C, "CU_" + name), name
        assert f"ICAR_CU_{name}={n}" in mod
    assert ids["ICAR_CU_N"] == len(ARRAYS) == C.CU_N and f"ICAR_CU_N={len(ARRAYS)}" in mod
    assert sorted(C.CU_NAMES.values()) == list(range(len(ARRAYS)))
    assert ids["ICAR_CU_BMJ"] == 5 == K.kCU_BMJ and "ICAR_CU_BMJ = 5" in mod
    assert "#define ICAR_CU_NO_STOCHASTIC (-9999.0f)" in hdr and K.kNO_STOCHASTIC == -9999 and "ICAR_CU_NO_STOCHASTIC = -9999.0" in mod
    assert (K.kCU_TIEDTKE, K.kCU_SIMPLE, K.kCU_KAINFR, K.kCU_NSAS) == (1, 2, 3, 4)
    # the slot's arrays took no field id
    assert ids["ICAR_N_FIELD_SLOTS"] == 63 == F.N_FIELD_SLOTS == max(F.NAMES.values()) + 1


def test_cu_configure_refusals_without_a_device():
    L = _lib()
    err = lambda: L.icar_hip_last_error().decode()
    fr = (1.0, -1.0, -1.0, -1.0, -1.0)
    assert L.icar_hip_cu_configure(None, 1, NO_STOCH, *fr) != 0 and "kCU_TIEDTKE" in err() and "not built" in err(), err()
    assert L.icar_hip_cu_configure(None, 4, NO_STOCH, *fr) != 0 and "kCU_NSAS" in err() and "not built" in err(), err()
    assert L.icar_hip_cu_configure(None, 2, NO_STOCH, *fr) != 0 and "kCU_SIMPLE" in err() and "no branch" in err(), err()
    assert L.icar_hip_cu_configure(None, 3, NO_STOCH, *fr) != 0 and "kCU_KAINFR" in err() and "commented out" in err(), err()
    assert L.icar_hip_cu_configure(None, 6, NO_STOCH, *fr) != 0 and "convection is 0 or 5" in err(), err()
    assert L.icar_hip_cu_configure(None, -1, NO_STOCH, *fr) != 0 and "convection is 0 or 5" in err(), err()
    assert L.icar_hip_cu_configure(None, 5, 20.0, *fr) != 0 and "random_number" in err() and "stochastic_cu" in err(), err()
    assert L.icar_hip_cu_configure(None, 5, NO_STOCH, float("nan"), -1.0, -1.0, -1.0, -1.0) != 0 and "NaN" in err(), err()
    # the value refusals come first; only then the context
    assert L.icar_hip_cu_configure(None, 5, NO_STOCH, *fr) != 0 and "null ctx" in err(), err()
    assert L.icar_hip_cu_configure(None, 0, NO_STOCH, *fr) != 0 and "null ctx" in err(), err()
    for fn, args in ((L.icar_hip_cu_bmj, (60.0, 2, 3, 2, 3)), (L.icar_hip_convect, (60.0,)), (L.icar_hip_cu_reset, ()),
                     (L.icar_hip_cu_upload, (0, None)), (L.icar_hip_cu_download, (0, None)), (L.icar_hip_cu_tables, (None, 0, None))):
        assert fn(None, *args) != 0 and "null argument" in err(), err()


def test_level_counts_are_refused_before_any_launch():
    """too few levels (the access is named), kts /= 1 and too many levels: the checks sit in front of every launch of the scheme, in
    icar_hip_cu_bmj and in icar_hip_convect alike; the restatement refuses the same counts"""
    import bmj_oracle as B
    import pytest
    src = open(os.path.join(ROOT, "icar_amd", "csrc", "cu_bmj.hip")).read()
    for fn in ("int icar_cu_bmj_run(", "int icar_convect_run("):
        body = src[src.index(fn):]
        assert body.index("levels_ok(") < body.index("hipLaunchKernelGGL("), fn
    chk = src[src.index("int levels_ok("):src.index("int tile_ok(")]
    assert "PRSMID(LBOT+1)" in chk and "cu_bmj.f90:755" in chk and "at least 3" in chk
    assert "kts != 1" in chk and "DTDT(1)" in chk and "cu_bmj.f90:248" in chk
    assert "BMJ_MAX_LEVELS" in chk and "at most" in chk
    assert B.MIN_NZ == 3 and B.MAX_LEVELS() == 128
    c = B.make_case(nx=6, ny=5, nz=4, seed=11)
    for kte in (1, 2):
        with pytest.raises(ValueError, match="level count refused"):
            B.drv(c, B.state(c), 20.0, kte=kte)
    B.drv(c, B.state(c), 20.0, kte=3)


def test_python_mirror_names_and_defaults():
    import inspect
    from icar_amd import convection, time_step
    from icar_amd.options import options_t
    for n in ("cu_var_request", "init_convection", "convect", "cu_bmj", "cu_configure", "cu_reset", "cu_get", "cu_set", "cu_tables"):
        assert callable(getattr(convection, n))
    opt = options_t()
    assert opt.physics.convection == 0
    o = opt.cu_options                                                  # options_obj.f90:1630-1649
    assert (o.stochastic_cu, o.tendency_fraction, o.tend_qv_fraction, o.tend_qc_fraction, o.tend_th_fraction, o.tend_qi_fraction) == \
        (-9999.0, 1.0, -1.0, -1.0, -1.0, -1.0)
    assert o.resolved() == (1.0, 1.0, 1.0, 1.0)
    o.tendency_fraction, o.tend_th_fraction = 0.5, 0.0
    assert o.resolved() == (0.5, 0.5, 0.0, 0.5)
    convection.cu_var_request(opt)
    assert not opt.vars_to_allocate                                     # convection = 0 requests nothing
    opt.physics.convection = K.kCU_BMJ
    convection.cu_var_request(opt)                                      # cu_driver.f90:75-89
    assert len(opt.vars_to_allocate) == 27 and {"kpbl", "tend_qv", "tend_th", "land_mask", "pressure_interface", "dz_interface"} <= set(opt.vars_to_allocate)
    assert set(opt.vars_to_advect) == {"potential_temperature", "water_vapor"}
    assert len(opt.vars_for_restart) == 13 and "kpbl" in opt.vars_for_restart and "tend_qv" not in opt.vars_for_restart
    assert "convection=0" in inspect.getsource(time_step.mp_and_halo) and "[convect]" in time_step.step.__doc__
    assert "convection=None" in inspect.getsource(__import__("icar_amd.domain", fromlist=["domain_t"]).domain_t.configure)

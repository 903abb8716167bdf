"""The surface-flux entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the
Fortran module, exported by the library; the new field ids behind an unchanged ICAR_N_FIELD_IDS; every refusal that needs no
context, with its message; the Python mirror.  (A context needs a device: the library's refusal of a surface layer that reaches
kte is in tests/test_gpu_sfc_columns.py; here the message is held in the source and the restatement refuses the same call.)"""
import os
import re
import subprocess

import pytest

from icar_amd import capi, _fields as F, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_lsm_configure", "icar_hip_diag_10m", "icar_hip_water_simple", "icar_hip_apply_fluxes", "icar_hip_lsm", "icar_hip_lsm_layers"]
NAMES = ["ROUGHNESS_Z0", "U_10M", "V_10M", "USTAR", "SST", "SKIN_TEMPERATURE", "SENSIBLE_HEAT", "LATENT_HEAT", "QSFC", "QFX", "DZ_INTERFACE"]


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
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    L = _lib()
    for n, name in enumerate(NAMES):
        assert ids["ICAR_F_" + name] == 52 + n == getattr(F, name) == F.NAMES[name.lower()], name
        assert f"ICAR_F_{name}={52 + n}" in mod
        assert L.icar_hip_field_elem_size(52 + n) == 4                     # REAL(4)
    # the older bounds stay where hosts and the older tests have them; the new one is the one the entry points check
    assert ids["ICAR_N_FIELD_IDS"] == 52 == F.N_FIELD_IDS and ids["ICAR_N_FIELDS"] == 47 == F.N_FIELDS
    assert ids["ICAR_N_FIELD_SLOTS"] == 63 == F.N_FIELD_SLOTS == max(F.NAMES.values()) + 1
    for src in ("capi.hip", "ctx.h", "step.hip", "halo_pack.hip"):
        text = open(os.path.join(ROOT, "icar_amd", "csrc", src)).read()
        assert "ICAR_N_FIELD_IDS" not in text, f"{src} still bounds an id by ICAR_N_FIELD_IDS"
    assert ids["ICAR_LSM_BASIC"] == 1 == K.kLSM_BASIC and ids["ICAR_WATER_SIMPLE"] == 2 == K.kWATER_SIMPLE
    assert (K.kLSM_SIMPLE, K.kLSM_NOAH, K.kLSM_NOAHMP, K.kWATER_BASIC, K.kWATER_LAKE) == (2, 3, 4, 1, 3)


def test_lsm_configure_refusals_without_a_device():
    L = _lib()
    err = lambda: L.icar_hip_last_error().decode()
    ok = (300, 0.625, 1.0, 400.0)
    assert L.icar_hip_lsm_configure(None, 2, 0, *ok) != 0
    assert "Simple LSM not settup, choose a different LSM options" in err() and "kLSM_SIMPLE" in err(), err()
    assert L.icar_hip_lsm_configure(None, 3, 0, *ok) != 0 and "kLSM_NOAH)" in err() and "not built" in err(), err()
    assert L.icar_hip_lsm_configure(None, 4, 2, *ok) != 0 and "kLSM_NOAHMP" in err() and "not built" in err(), err()
    assert L.icar_hip_lsm_configure(None, 1, 3, *ok) != 0 and "kWATER_LAKE" in err() and "not built" in err(), err()
    assert L.icar_hip_lsm_configure(None, 7, 0, *ok) != 0 and "landsurface is 0 or 1" in err()
    assert L.icar_hip_lsm_configure(None, 1, -1, *ok) != 0 and "watersurface is 0, 1" in err()
    assert L.icar_hip_lsm_configure(None, 1, 2, -5, 0.625, 1.0, 400.0) != 0 and "update_interval" in err()
    assert L.icar_hip_lsm_configure(None, 1, 2, 300, 0.625, 1.0, 0.0) != 0 and "sfc_layer_thickness" in err()
    assert L.icar_hip_lsm_configure(None, 1, 2, *ok) != 0 and "null ctx" in err()
    for fn, args in ((L.icar_hip_diag_10m, ()), (L.icar_hip_water_simple, ()), (L.icar_hip_apply_fluxes, (60.0, 2, 3, 2, 3, 1, 4)), (L.icar_hip_lsm, (60.0,)),
                     (L.icar_hip_lsm_layers, (None,))):
        assert fn(None, *args) != 0 and "null argument" in err(), err()


def test_layer_that_reaches_kte_is_refused_before_any_launch():
    import sfc_oracle as S
    src = open(os.path.join(ROOT, "icar_amd", "csrc", "sfc_basic.hip")).read()
    body = src[src.index("int icar_sfc_apply_fluxes_run("):]
    check, launch = body.index("the surface layer reaches kte"), body.index("hipLaunchKernelGGL(k_apply_fluxes")
    assert check < launch and "reads out of bounds" in body[:launch], "the refusal comes before the launch and says why"
    c = S.make_case(8, 6, 3, seed=9)
    with pytest.raises(ValueError, match="reaches past kte"):
        S.run_oracle(c, S.state(c))


def test_python_mirror_names():
    from icar_amd import surface
    from icar_amd.options import options_t
    for n in ("lsm_var_request", "lsm_init", "lsm", "water_simple", "apply_fluxes", "diag_10m", "lsm_layers", "lsm_configure"):
        assert callable(getattr(surface, n))
    opt = options_t()
    assert (opt.physics.landsurface, opt.physics.watersurface) == (0, 0)
    o = opt.lsm_options
    assert (o.update_interval, o.sh_feedback_fraction, o.lh_feedback_fraction, o.sfc_layer_thickness) == (300, 0.625, 1.0, 400.0)
    opt.physics.landsurface, opt.physics.watersurface = K.kLSM_BASIC, K.kWATER_SIMPLE
    surface.lsm_var_request(opt)                    # kLSM_BASIC and kWATER_SIMPLE request nothing in the reference either
    assert not opt.vars_to_allocate and not opt.vars_to_advect and not opt.vars_for_restart
    import inspect
    from icar_amd import time_step
    assert "landsurface=0" in inspect.getsource(time_step.mp_and_halo) and "[lsm]" in time_step.step.__doc__

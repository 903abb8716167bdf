"""The radiation entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the
Fortran module, exported by the library; the field ids; the argument checks that need no context; the calendar anchor's integer
date arithmetic against hand-computed values.  (A context needs a device: the library's refusal of fewer than 5 levels is in
tests/test_gpu_ra_columns.py; here the message is held in the source and the restatement refuses the same call.)"""
import os
import re
import subprocess

import pytest

from icar_amd import capi, _fields as F, constants as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_ra_simple", "icar_hip_rad_configure", "icar_hip_rad_calendar", "icar_hip_rad"]


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
    names = ["LATITUDE", "LONGITUDE", "SHORTWAVE", "LONGWAVE", "CLOUD_FRACTION"]
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    L = _lib()
    for n, name in enumerate(names):
        assert ids["ICAR_F_" + name] == 47 + n == getattr(F, name) == F.NAMES[name.lower()], name
        assert f"ICAR_F_{name}={47 + n}" in mod
        assert L.icar_hip_field_elem_size(47 + n) == 4                     # REAL(4)
    assert ids["ICAR_N_FIELD_IDS"] == 52 == F.N_FIELD_IDS and ids["ICAR_N_FIELDS"] == 47 == F.N_FIELDS and ids["ICAR_RA_SIMPLE"] == 2 == K.kRA_SIMPLE
    assert (K.kRA_BASIC, K.kRA_RRTMG) == (1, 3)


def test_rad_configure_refuses_rrtmg_without_a_device():
    L = _lib()
    assert L.icar_hip_rad_configure(None, 3) != 0
    msg = L.icar_hip_last_error().decode()
    assert "RRTMG" in msg and "not built" in msg, msg
    assert L.icar_hip_rad_configure(None, 7) != 0 and "radiation is 0, 1" in L.icar_hip_last_error().decode()
    assert L.icar_hip_rad_configure(None, 2) != 0 and "null ctx" in L.icar_hip_last_error().decode()
    assert L.icar_hip_rad_calendar(None, 5, 0.0, 365.0, 365.0) != 0 and "calendar is 0" in L.icar_hip_last_error().decode()
    assert L.icar_hip_rad_calendar(None, 0, 0.0, 0.0, 365.0) != 0 and "positive" in L.icar_hip_last_error().decode()


def test_fewer_than_five_levels_is_refused():
    import numpy as np
    import ra_oracle as R
    src = open(os.path.join(ROOT, "icar_amd", "csrc", "ra_simple.hip")).read()
    check, launch = src.index('"ra_simple: at least 5 levels'), src.index("hipLaunchKernelGGL(k_ra_")
    assert check < launch, "the refusal comes before any launch"
    c = R.make_case(8, 6, 4, seed=9)
    with pytest.raises(ValueError, match="ra_simple: at least 5 levels"):
        R.run_oracle(c, R.state(c))
    c = R.make_case(8, 6, 7, seed=9)
    with pytest.raises(ValueError, match="at least 5 levels"):
        R.run_oracle(c, R.state(c), kts=4)                                  # kts + 4 > nz
    R.run_oracle(c, R.state(c), kts=3, kte=5)                               # three levels of hydrometeors, five of T_air: fine


def test_calendar_anchor_hand_computed():
    from icar_amd.radiation import calendar_anchor, GREGORIAN, NOLEAP, THREESIXTY
    # 2000-03-01 12:00: January 31 + February 29 (a leap year) = day 60.5 of 366; without leap years 59.5 of 365
    assert calendar_anchor(2000, 3, 1, 12, 0, 0, GREGORIAN) == (60 * 86400 + 43200, 366, 365)
    assert calendar_anchor(2000, 3, 1, 12, 0, 0, NOLEAP) == (59 * 86400 + 43200, 365, 365)
    assert calendar_anchor(2000, 3, 1, 12, 0, 0, THREESIXTY) == (60 * 86400 + 43200, 360, 360)      # 2 x 30 days
    assert calendar_anchor(1900, 3, 1, 0, 0, 0, GREGORIAN) == (59 * 86400, 365, 365)                 # 1900 is no leap year
    assert calendar_anchor(2023, 12, 31, 23, 59, 59, GREGORIAN) == (365 * 86400 - 1, 365, 366)
    assert calendar_anchor(2024, 1, 1) == (0, 366, 365)
    assert calendar_anchor(2001, 12, 30, 6, 30, 15, THREESIXTY) == (359 * 86400 + 6 * 3600 + 30 * 60 + 15, 360, 360)
    with pytest.raises(ValueError):
        calendar_anchor(2000, 1, 1, calendar=3)


def test_python_mirror_names():
    from icar_amd import radiation
    from icar_amd.options import options_t
    for n in ("ra_var_request", "rad_init", "rad", "ra_simple", "calendar_anchor", "rad_calendar"):
        assert callable(getattr(radiation, n))
    opt = options_t()
    assert opt.physics.radiation == 0
    radiation.ra_var_request(opt)
    assert not opt.vars_to_allocate and not opt.vars_to_advect
    opt.physics.radiation = K.kRA_SIMPLE
    radiation.ra_var_request(opt)
    assert opt.vars_to_advect == {"potential_temperature": 1}
    assert set(opt.vars_to_allocate) == {"pressure", "potential_temperature", "exner", "cloud_fraction", "water_vapor", "cloud_water", "rain_in_air",
                                         "snow_in_air", "shortwave", "longwave", "cloud_ice", "graupel_in_air"}
    assert set(opt.vars_for_restart) == {"pressure", "potential_temperature", "shortwave", "longwave", "cloud_fraction"}

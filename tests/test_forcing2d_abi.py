"""The entry points of the 2-D forced variables (include/icar_hip.h, F3): the header, the ctypes binding, the Fortran module and the
library's dynamic symbol table agree on the names, the enum and the signatures.  CPU only.  The refusals come behind the context, which
needs a device (tests/test_gpu_forcing2d.py has them); without one every entry point refuses the null context by its own name
(tests/test_abi.py::test_entry_points_refuse_a_null_context covers every symbol of the binding, these included)."""
import ctypes
import os
import re
import subprocess

from icar_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["icar_hip_forcing2d_upload", "icar_hip_forcing2d_download", "icar_hip_interpolate_forcing_2d", "icar_hip_update_delta_fields_2d",
       "icar_hip_apply_forcing_2d", "icar_hip_forcing2d_enable", "icar_hip_forcing2d_get", "icar_hip_forcing2d_set"]
FORTRAN = ["hip_forcing2d_upload", "hip_forcing2d_download", "hip_forcing2d_interpolate", "hip_forcing2d_update_delta", "hip_forcing2d_apply",
           "hip_forcing2d_enable", "hip_forcing2d_get", "hip_forcing2d_set"]
ENUM = {"ICAR_FORCED2D_SST": 0, "ICAR_FORCED2D_SHORTWAVE": 1, "ICAR_FORCED2D_LONGWAVE": 2, "ICAR_FORCED2D_EXTERNAL_PRECIPITATION": 3,
        "ICAR_FORCED2D_N": 4, "ICAR_FORCED2D_DATA": 0, "ICAR_FORCED2D_DQDT": 1}


def header():
    return open(os.path.join(ROOT, "include", "icar_hip.h")).read()


def code():
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def test_header_binding_and_library_agree():
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code()), s
        assert s in capi.SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        from icar_amd import build
        build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported
    L = capi.lib()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    ip = ctypes.POINTER(ci)
    want = {"icar_hip_forcing2d_upload": [vp, ci, vp, ci, ci], "icar_hip_forcing2d_download": [vp, ci, vp, ctypes.c_size_t],
            "icar_hip_interpolate_forcing_2d": [vp, ip, ci, ci], "icar_hip_update_delta_fields_2d": [vp, ip, ci, cd],
            "icar_hip_apply_forcing_2d": [vp, cd], "icar_hip_forcing2d_enable": [vp, ip, ci], "icar_hip_forcing2d_get": [vp, ci, ci, vp],
            "icar_hip_forcing2d_set": [vp, ci, ci, vp]}
    ctype = {"icar_hip_ctx *": vp, "int": ci, "double": cd, "size_t": ctypes.c_size_t, "const float *": vp, "float *": vp, "const int *": ip}
    for s in NEW:
        assert getattr(L, s).argtypes == want[s], s
        # ... and the header's parameter list is that signature
        params = re.search(r"\bint\s+" + s + r"\s*\((.*?)\)\s*;", code(), flags=re.S).group(1)
        types = [re.sub(r"\s*\b\w+$", "", q.strip()).strip() for q in params.split(",")]
        assert [ctype[t] for t in types] == want[s], (s, types)


def test_the_enum_and_the_slot_count():
    body = re.search(r"typedef enum icar_hip_forced2d \{(.*?)\} icar_hip_forced2d;", code(), flags=re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(ICAR_FORCED2D_\w+)\s*=\s*(\d+)", body)}
    assert vals == {k: v for k, v in ENUM.items() if k not in ("ICAR_FORCED2D_DATA", "ICAR_FORCED2D_DQDT")}
    assert re.search(r"enum\s*\{\s*ICAR_FORCED2D_DATA\s*=\s*0\s*,\s*ICAR_FORCED2D_DQDT\s*=\s*1\s*\}", code())
    assert vals["ICAR_FORCED2D_N"] == 4 == capi.FORCED2D_N == len(capi.FORCED2D)
    assert capi.FORCED2D == {"sst": 0, "shortwave": 1, "longwave": 2, "external_precipitation": 3}
    assert (capi.FORCED2D_DATA, capi.FORCED2D_DQDT) == (0, 1)
    assert re.search(r"ICAR_N_FIELD_SLOTS\s*=\s*63\b", code())
    # no field id moved: the three slots the family writes are where they were
    for name, v in (("ICAR_F_SHORTWAVE", 49), ("ICAR_F_LONGWAVE", 50), ("ICAR_F_SST", 56), ("ICAR_F_PRECIPITATION", 23)):
        assert re.search(name + r"\s*=\s*%d\b" % v, code()), name


def test_fortran_module_binds_the_entry_points():
    f90 = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    for s in NEW:
        assert f'name="{s}"' in f90.replace("name = ", "name=").replace("'", '"'), s
    public = f90[:f90.index("type, bind(C) :: forcing_geo_c")]
    for s in FORTRAN:
        assert re.search(r"subroutine\s+" + s + r"\b", f90), s
        assert re.search(r"\b" + s + r"\b", public), s + " is not public"
    for k, v in ENUM.items():
        assert re.search(r"\b" + k + r"\s*=\s*%d\b" % v, f90), k
        assert re.search(r"\b" + k + r"\b", public), k + " is not public"


def test_every_entry_cites_what_it_replaces():
    block = header()[header().index("---- F3:"):]
    block = block[:block.index("int icar_hip_forcing2d_set")]
    for cite in ("domain_obj.f90:199, :212, :215, :272", "domain_obj.f90:2595-2600", "geo_reader.f90:1142-1182", "domain_obj.f90:2355-2356",
                 "domain_obj.f90:2400-2402", ":2438-2445", "time_step.f90:534"):
        assert cite in block, cite

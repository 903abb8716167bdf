"""The forcing update's entry points (include/icar_hip.h, F2): the header, the ctypes binding, the Fortran module and the library's
dynamic symbol table agree.  CPU only.  The refusals of forcing_configure come behind the context, which needs a device
(tests/test_gpu_forcing.py has them); without one every entry point refuses the null context by its own name
(tests/test_abi.py::test_entry_points_refuse_a_null_context covers every symbol of the binding, these included)."""
import ctypes
import os
import re
import subprocess

from icar_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["icar_hip_forcing_configure", "icar_hip_forcing_upload", "icar_hip_forcing_download", "icar_hip_interpolate_forcing",
       "icar_hip_update_delta_fields", "icar_hip_forcing_step"]


def header():
    return open(os.path.join(ROOT, "include", "icar_hip.h")).read()


def test_header_binding_and_library_agree():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert s in capi.SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        from icar_amd import build
        build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(NEW) <= exported
    L = capi.lib()
    gp = ctypes.POINTER(capi.forcing_geo_c)
    assert L.icar_hip_forcing_configure.argtypes[1:4] == [gp, gp, gp] and len(L.icar_hip_forcing_configure.argtypes) == 8
    assert len(L.icar_hip_forcing_step.argtypes) == 10 and L.icar_hip_forcing_step.argtypes[-1] is ctypes.c_double
    assert L.icar_hip_update_delta_fields.argtypes[-1] is ctypes.c_double


def test_struct_layout_is_the_header_s():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct icar_hip_forcing_geo \{(.*?)\} icar_hip_forcing_geo;", code, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(int|float)\s+", "", decl).split(",")]
    assert names == [n for n, _ in capi.forcing_geo_c._fields_]
    assert ctypes.sizeof(capi.forcing_geo_c) == 5 * ctypes.sizeof(ctypes.c_void_p) + 8 * 4          # 7 ints and the tail padding


def test_fortran_module_binds_the_entry_points():
    f90 = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    for s in NEW:
        assert f'name="{s}"' in f90.replace("name = ", "name=").replace("'", '"'), s
    for s in ("hip_forcing_configure", "hip_forcing_upload", "hip_interpolate_forcing", "hip_update_delta_fields", "hip_forcing_step"):
        assert re.search(r"subroutine\s+" + s + r"\b", f90), s


def test_every_entry_cites_what_it_replaces():
    block = header()[header().index("---- F2:"):]
    block = block[:block.index("int icar_hip_forcing_step")]
    for cite in ("driver.f90:133-137", "domain_obj.f90:2559-2643", ":2339-2372", "geo_reader.f90:1069-1136", "vinterp.f90:284-295",
                 "atm_utilities.f90:611-653", "time_delta_obj.f90:123-130", ":2656-2702"):
        assert cite in block, cite

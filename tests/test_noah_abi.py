"""The Noah entry points at the C-ABI level, without a GPU: declared in include/icar_hip.h, bound in icar_amd/capi.py and the Fortran
module, exported by the library; the enum of the model's arrays behind unchanged field ids; every refusal that needs no context, looked
at before the context; icar_hip_lsm_configure keeps refusing 3 and names icar_hip_lsm_init; the Python mirror; the Fortran binding
compiles (flang -fsyntax-only) together with a host-side caller that associates the tables with arrays of the reference's extents."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from icar_amd import capi, constants as K, surface
from icar_amd.build import FLANG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["icar_hip_noah_tables", "icar_hip_lsm_init", "icar_hip_lsm_noah", "icar_hip_noah_upload", "icar_hip_noah_download"]
OK = (300, ctypes.c_float(0.625), ctypes.c_float(1.0), ctypes.c_float(400.0))


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        from icar_amd import build
        build.build()
    return capi.lib()


def test_entry_points_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    L = _lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for s in ENTRY:
        assert re.search(r"\bint\s+" + s + r"\s*\(\s*icar_hip_ctx\s*\*\s*ctx\b", hdr), f"{s} is not declared with the context first in include/icar_hip.h"
        assert s in capi.SYMBOLS and hasattr(L, s) and s in exported, s
        assert f'bind(C, name="{s}")' in mod and ("hip_" + s[len("icar_hip_"):]) in mod, f"{s}: no Fortran binding"
    doc = text.split("---- L2:")[1].split("enum { ICAR_LSM_NOAH")[0]                  # each entry cites the lines it replaces
    for s, lines in (("icar_hip_noah_tables", "lsm_noahdrv.f90:1199-1432"), ("icar_hip_lsm_init", "lsm_driver.f90:522-711"),
                     ("icar_hip_lsm_noah", "lsm_driver.f90:1210-1278"), ("icar_hip_noah_upload", "ICAR_NOAH_")):
        assert s in doc and lines in doc, s
    assert ":425-520" in doc and ":674-675" in doc and "lsm_noahdrv.f90:1095-1188" in doc and ":887-901" in doc


def test_enum_values_agree_and_field_ids_stay():
    hdr = open(os.path.join(ROOT, "include", "icar_hip.h")).read()
    mod = open(os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICAR_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert ids["ICAR_LSM_NOAH"] == 3 == K.kLSM_NOAH and "ICAR_LSM_NOAH = 3" in mod
    for n, name in enumerate(surface.NOAH_ARRAYS):
        assert ids["ICAR_NOAH_" + name.upper()] == n == surface.NOAH_ID[name], name
        assert re.search(r"\bICAR_NOAH_" + name.upper() + r"=" + str(n) + r"\b", mod), name
    assert ids["ICAR_NOAH_N"] == len(surface.NOAH_ARRAYS) == 42 and re.search(r"ICAR_NOAH_N=42\b", mod)
    assert ids["ICAR_N_FIELDS"] == 47 and ids["ICAR_N_FIELD_IDS"] == 52 and ids["ICAR_N_FIELD_SLOTS"] == 63
    assert ids["ICAR_CU_N"] == 7 and ids["ICAR_NSAS_N"] == 6 and ids["ICAR_YSU_N"] == 19
    # the structs' layouts: the C header, the ctypes mirror and the cell header name the same members in the same order
    col = open(os.path.join(ROOT, "icar_amd", "csrc", "noah_column.h")).read()
    members = lambda body: re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    c_tab = members(hdr.split("typedef struct icar_hip_noah_tables_t {")[1].split("}")[0])
    h_tab = members(col.split("typedef struct {\n    const int *nrotbl;")[1].split("} NoahTables;")[0])
    py_tab = [n for n, _ in capi.noah_tables_c._fields_]
    assert c_tab == py_tab and ["nrotbl"] + h_tab == py_tab, (c_tab, h_tab, py_tab)
    c_opt = members(hdr.split("typedef struct icar_hip_noah_options_t {")[1].split("}")[0])
    assert c_opt == [n for n, _ in capi.noah_options_c._fields_]


def tables_struct(lucats=21, slcats=19, slpcats=9, bare=16, nroot=3):
    t = capi.noah_tables_c()
    keep = [(ctypes.c_int * 50)(*[nroot] * 50)] + [(ctypes.c_float * 50)(*[0.5] * 50) for _ in range(25)]
    t.nrotbl = ctypes.addressof(keep[0])
    for n, a in zip(capi.NOAH_T_VEG + capi.NOAH_T_SOIL + ["slope_data"], keep[1:]):
        setattr(t, n, ctypes.addressof(a))
    t.bare, t.lucats, t.slcats, t.slpcats = bare, lucats, slcats, slpcats
    t._keep = keep
    return t


def test_refusals_without_a_device():
    L = _lib()
    err = lambda: L.icar_hip_last_error().decode()
    o = capi.noah_options_c(13, 15, 17, 21, 0, 0, 0, 1e10)
    init = lambda ls, ws=0, opt=o, ok=OK: L.icar_hip_lsm_init(None, ls, ws, *ok, ctypes.byref(opt) if opt is not None else None)
    # the values are looked at before the context
    assert init(3) != 0 and err().startswith("lsm_init: ") and "null ctx" in err()
    assert init(4) != 0 and "kLSM_NOAHMP" in err() and "not built" in err() and "null ctx" not in err()
    assert init(3, 3) != 0 and "kWATER_LAKE" in err() and "not built" in err()
    assert init(3, -1) != 0 and "watersurface is 0, 1" in err()
    assert init(3, 0, o, (-5, OK[1], OK[2], OK[3])) != 0 and "update_interval" in err()
    assert init(3, 0, None) != 0 and "icar_hip_noah_options_t" in err()
    for member in ("monthly_vegfrac", "monthly_albedo"):
        bad = capi.noah_options_c(13, 15, 17, 21, 0, 0, 0, 1e10); setattr(bad, member, 1)
        assert init(3, 0, bad) != 0 and "monthly_vegfrac / monthly_albedo" in err() and "not built" in err()
    assert init(3, 0, capi.noah_options_c(0, 15, 17, 21, 0, 0, 0, 1e10)) != 0 and "urban_category" in err()
    assert init(3, 0, capi.noah_options_c(13, 15, 17, 21, 0, 0, 0, 0.0)) != 0 and "max_swe" in err()
    # 0, 1 and 2 do what icar_hip_lsm_configure does, with or without the options; the messages name this entry point
    assert init(1, 2, None) != 0 and err().startswith("lsm_init: ") and "null ctx" in err()
    assert init(0) != 0 and "null ctx" in err()
    assert init(2) != 0 and "Simple LSM not settup" in err() and err().startswith("lsm_init: ")
    assert init(7) != 0 and "landsurface is 0 or 1" in err()
    assert L.icar_hip_noah_tables(None, None) != 0 and err().startswith("noah_tables: ") and "null argument" in err()
    assert L.icar_hip_noah_tables(None, ctypes.byref(tables_struct())) != 0 and "null ctx" in err()
    for kw, word in ((dict(lucats=51), "LUCATS"), (dict(lucats=0), "LUCATS"), (dict(slcats=31), "SLCATS"), (dict(slpcats=0), "SLPCATS"), (dict(nroot=5), "NROTBL"),
                     (dict(bare=22), "BARE")):
        assert L.icar_hip_noah_tables(None, ctypes.byref(tables_struct(**kw))) != 0 and word in err() and "null ctx" not in err(), kw
    holed = tables_struct(); holed.satpsi = None
    assert L.icar_hip_noah_tables(None, ctypes.byref(holed)) != 0 and "pointer is null" in err() and "null ctx" not in err()
    holed = tables_struct(); holed.nrotbl = None
    assert L.icar_hip_noah_tables(None, ctypes.byref(holed)) != 0 and "pointer is null" in err()
    cf = ctypes.c_float
    assert L.icar_hip_lsm_noah(None, cf(0.0), 1, 1, 1, 1) != 0 and "lsm_dt is positive" in err()
    assert L.icar_hip_lsm_noah(None, cf(600.0), 1, 1, 1, 1) != 0 and err().startswith("lsm_noah: ") and "null argument" in err()
    buf = (ctypes.c_float * 4)()
    assert L.icar_hip_noah_upload(None, 0, buf) != 0 and err().startswith("noah_upload: ")
    assert L.icar_hip_noah_download(None, 0, buf) != 0 and err().startswith("noah_download: ")


def test_lsm_configure_keeps_refusing_noah_and_names_lsm_init():
    L = _lib()
    assert L.icar_hip_lsm_configure(None, 3, 0, *OK) != 0
    e = L.icar_hip_last_error().decode()
    assert "kLSM_NOAH)" in e and "not built" in e and "icar_hip_lsm_init" in e and e.startswith("lsm_configure: ")
    src = open(os.path.join(ROOT, "icar_amd", "csrc", "sfc_basic.hip")).read()
    assert "Noah runs through icar_hip_lsm_noah only" in src.split("int icar_lsm_run(")[1].split("const double now")[0], "lsm() says what is not built before its gate"


def test_python_mirror():
    from icar_amd.options import options_t
    for n in ("noah_tables", "noah_init", "lsm_noah", "noah_set", "noah_get", "lsm_init", "lsm", "lsm_configure"):
        assert callable(getattr(surface, n))
    o = options_t().lsm_options
    assert (o.urban_category, o.ice_category, o.water_category, o.lake_category) == (13, 15, 17, 21) and o.LU_Categories == "MODIFIED_IGBP_MODIS_NOAH"
    assert (o.monthly_vegfrac, o.monthly_albedo, o.update_interval, o.sfc_layer_thickness) == (False, False, 300, 400.0)
    assert surface.NOAH_ID["soil_water_content"] == 38 and surface.NOAH_ARRAYS[-4:] == ["soil_water_content", "soil_temperature", "sh2o", "smcrel"]


GLUE = """
! what a host does after the reference's own SOIL_VEG_GEN_PARM: associate the tables, upload the domain's arrays, lsm_init, lsm_noah
module noah_tables_stand_in
  integer, parameter :: NLUS = 50, NSLTYPE = 30, NSLOPE = 30
  integer, target :: NROTBL(NLUS), BARE, LUCATS, SLCATS, SLPCATS
  real, target, dimension(NLUS) :: SNUPTBL, RSTBL, RGLTBL, HSTBL, MAXALB, EMISSMINTBL, EMISSMAXTBL, LAIMINTBL, LAIMAXTBL, Z0MINTBL, Z0MAXTBL, &
                                   ALBEDOMINTBL, ALBEDOMAXTBL
  real, target, dimension(NSLTYPE) :: BB, DRYSMC, F11, MAXSMC, REFSMC, SATPSI, SATDK, SATDW, WLTSMC, QTZ
  real, target :: SLOPE_DATA(NSLOPE)
  real :: TOPT_DATA, CMCMAX_DATA, CFACTR_DATA, RSMAX_DATA, SBETA_DATA, FXEXP_DATA, CSOIL_DATA, SALP_DATA, REFDK_DATA, REFKDT_DATA, FRZK_DATA, ZBOT_DATA, LVCOEF_DATA
end module
subroutine noah_glue(ctx, veg_type, soil_temperature, chs, lsm_dt, its, ite, jts, jte)
  use icar_hip
  use noah_tables_stand_in
  implicit none
  type(hip_ctx_t), intent(in) :: ctx
  integer, intent(in) :: veg_type(:,:), its, ite, jts, jte
  real, intent(inout) :: soil_temperature(:,:,:), chs(:,:)
  real, intent(in) :: lsm_dt
  type(hip_noah_tables_t) :: t
  type(hip_noah_options_t) :: o
  t%nrotbl => NROTBL; t%snuptbl => SNUPTBL; t%rstbl => RSTBL; t%rgltbl => RGLTBL; t%hstbl => HSTBL; t%maxalb => MAXALB
  t%emissmintbl => EMISSMINTBL; t%emissmaxtbl => EMISSMAXTBL; t%laimintbl => LAIMINTBL; t%laimaxtbl => LAIMAXTBL; t%z0mintbl => Z0MINTBL
  t%z0maxtbl => Z0MAXTBL; t%albedomintbl => ALBEDOMINTBL; t%albedomaxtbl => ALBEDOMAXTBL
  t%bb => BB; t%drysmc => DRYSMC; t%f11 => F11; t%maxsmc => MAXSMC; t%refsmc => REFSMC; t%satpsi => SATPSI; t%satdk => SATDK; t%satdw => SATDW
  t%wltsmc => WLTSMC; t%qtz => QTZ; t%slope_data => SLOPE_DATA
  t%topt_data = TOPT_DATA; t%cmcmax_data = CMCMAX_DATA; t%cfactr_data = CFACTR_DATA; t%rsmax_data = RSMAX_DATA; t%sbeta_data = SBETA_DATA
  t%fxexp_data = FXEXP_DATA; t%csoil_data = CSOIL_DATA; t%salp_data = SALP_DATA; t%refdk_data = REFDK_DATA; t%refkdt_data = REFKDT_DATA
  t%frzk_data = FRZK_DATA; t%zbot_data = ZBOT_DATA; t%lvcoef_data = LVCOEF_DATA
  t%bare = BARE; t%lucats = LUCATS; t%slcats = SLCATS; t%slpcats = SLPCATS
  call hip_noah_tables(ctx, t)
  call hip_noah_upload_int(ctx, ICAR_NOAH_VEG_TYPE, veg_type)
  call hip_noah_upload(ctx, ICAR_NOAH_SOIL_TEMPERATURE, soil_temperature)
  o%fndsnowh = 1
  call hip_lsm_init(ctx, ICAR_LSM_NOAH, ICAR_WATER_SIMPLE, 300, 0.625, 1.0, 400.0, o)
  call hip_noah_upload(ctx, ICAR_NOAH_CHS, chs)
  call hip_lsm_noah(ctx, lsm_dt, its, ite, jts, jte)
  call hip_noah_download(ctx, ICAR_NOAH_SOIL_TEMPERATURE, soil_temperature)
end subroutine
"""


@pytest.mark.skipif(not (os.path.exists(FLANG) or shutil.which(FLANG)), reason="flang is not present on this host")
def test_fortran_binding_and_a_host_caller_compile(tmp_path):
    mod = os.path.join(ROOT, "icar_amd", "fortran", "icar_hip_mod.f90")
    run = lambda path: subprocess.run([FLANG, "-fsyntax-only", "-I" + str(tmp_path), "-module-dir", str(tmp_path), path], capture_output=True, text=True)
    r = run(mod)
    assert r.returncode == 0, r.stderr[-3000:]
    glue = tmp_path / "noah_glue.f90"
    glue.write_text(GLUE)
    r = run(str(glue))
    assert r.returncode == 0, r.stderr[-3000:]

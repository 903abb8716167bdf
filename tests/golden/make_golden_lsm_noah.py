#!/usr/bin/env python
"""Golden vectors of the Noah branch of lsm() under tests/golden/lsm_noah_*.npz made by RUNNING THE REFERENCE'S OWN CODE, compiled with
the flang and the flags of oracle/build_ref.sh in a temporary directory outside the repository:

  lsm_noah, LSM_NOAH_INIT  src/physics/lsm_noahlsm.f90 and src/physics/lsm_noahdrv.f90 WHOLE AND UNMODIFIED behind the shim of
                           tests/golden/make_golden_noah.py, called with lsm_driver.f90's arguments
  sat_mr                   src/utilities/atm_utilities.f90 WHOLE AND UNMODIFIED (with the interface modules it uses)
  the statements of lsm()  src/physics/lsm_driver.f90, EXCERPTED BY THEIR TEXT at generation time into a shim module of the generator's
  and lsm_init             own (nothing of the reference is committed): the subroutines calc_exchange_coefficient and
                           surface_diagnostics, and the statements :566, :584, :593, :596, :603, :610-611, :992-997 of lsm_init and :1028,
                           :1030, :1144-1147, :1181-1187, :1207, :1280-1290, :1524-1527, :1530-1545 of lsm.  lsm_driver.f90 as a whole
                           uses Noah-MP, the lake model and a live domain_t with coarray members, which nothing here can build or run.
                           The shim's domain_t holds `real, pointer` arrays under the reference's member names; the module's own arrays
                           (Z0, Ri, CHS, RAINBL, ...) are pointers to the generator's buffers.  temperature_2m_bare is not associated,
                           as lsm_var_request leaves it for Noah.  The line numbers are only checked to lie within 40 lines.
The gate (REAL(8) clock arithmetic, :1016-1023) is four lines of control flow and is restated (tests/lsm_noah_driver_oracle.py: gate), as
in make_golden_sfc.py; the order of the pieces inside the gated block is lsm()'s: windspd, calc_exchange_coefficient, CHS * windspd, QGH,
current_precipitation, lsm_noah, the statements behind it, soil_totalmoisture, surface_diagnostics.  LSM_NOAH_INIT and lsm_noah run on the
tile 2..nx-1, 2..ny-1, everything else on what the reference's statements name.

LAND ICE.  On a land-ice cell lsm_noah stores locals that only SFLX sets in the arrays of noah_oracle.ICE_UNSET: the values of the cell
visited before (make_golden_noah.py shows it).  As that generator does for the carried state, these values are replaced by what the
restatement leaves there (the arrays unchanged) right behind lsm_noah; the statements behind the call then read defined values and
EVERY array is compared in EVERY cell.  The generator asserts that land ice is at most 5 % of each fixture's cells and prints the share.

Before anything is written the generator asserts, for every case of tests/lsm_noah_driver_oracle.py:CASES and the seeds of SEEDS,
  (0) the restatement (icar_amd/csrc/lsm_noah_driver_cell.h around noah_column.h) reproduces the compiled reference bit for bit after
      lsm_init and after every call in every array the block writes;
  (1) every stored value is finite;
  (2) one call of every case finds the gate shut and at least one cell inside a tile has wind == 0;
  (3) the coverage of lsm_noah_driver_oracle.REQUIRED: each arm in at least 2 % of the tile's cells in some call of some fixture; the
      arms of NOT_REACHED never occur;
and records whether the FMA-contracted build of the restatement differs from the reference (it should).
Only runs where the reference is present; tests/test_lsm_noah_driver_oracle.py pins the restatement to these files everywhere."""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import noah_oracle as N  # noqa: E402
import lsm_noah_driver_oracle as LN  # noqa: E402
import make_golden_noah as G  # noqa: E402
from make_golden_sfc import excerpt  # noqa: E402

REF = G.REF
FC = G.FC
f32, f64 = np.float32, np.float64
MODULES = ["constants/icar_constants", "constants/wrf_constants", "utilities/time_delta_obj", "utilities/time_h", "main/data_structures",
           "objects/opt_types", "objects/options_h", "physics/mp_thompson", "utilities/atm_utilities"]

# the buffers the shim's pointers name, in the order ref_lnd_bind takes them
BIND2 = [("znt", "dom%roughness_z0%data_2d"), ("z0", "Z0"), ("terrain", "dom%terrain%data_2d"), ("t2", "dom%temperature_2m%data_2d"),
         ("q2", "dom%humidity_2m%data_2d"), ("lwup", "dom%longwave_up%data_2d"), ("tsk", "dom%skin_temperature%data_2d"),
         ("snow", "dom%snow_water_equivalent%data_2d"), ("smstot", "dom%soil_totalmoisture%data_2d"), ("u10", "dom%u_10m%data_2d"),
         ("v10", "dom%v_10m%data_2d"), ("psfc", "dom%surface_pressure%data_2d"), ("hfx", "dom%sensible_heat%data_2d"),
         ("t2veg", "dom%temperature_2m_veg%data_2d"), ("rib", "Ri"), ("z_atm", "z_atm"), ("lnz", "lnz_atm_term"), ("base", "base_exchange_term"),
         ("rainbl_step", "current_precipitation"), ("windspd", "windspd"), ("chs", "CHS"), ("chs2", "CHS2"), ("cqs2", "CQS2"), ("qgh", "QGH"),
         ("emiss", "EMISS"), ("qfx", "QFX"), ("qsfc", "QSFC"), ("vegfra", "VEGFRAC")]
BIND2D = [("precip", "dom%accumulated_precipitation%data_2dd"), ("rainbl8", "RAINBL")]
BIND2I = [("land_mask", "dom%land_mask"), ("ivgtyp", "dom%veg_type")]
BIND3 = [("t3", "dom%temperature%data_3d", 2), ("qv3", "dom%water_vapor%data_3d", 2), ("z3", "dom%z%data_3d", 2), ("smois", "dom%soil_water_content%data_3d", 4)]

SHIM = """
module lnd_shim
  use iso_c_binding
  use icar_constants
  use mod_atm_utilities, only: sat_mr
  implicit none
  type v3_t
    real, pointer :: data_3d(:,:,:) => null()
  end type
  type v2_t
    real, pointer :: data_2d(:,:) => null()
    double precision, pointer :: data_2dd(:,:) => null()
  end type
  type domain_t
    type(v3_t) :: temperature, water_vapor, z, soil_water_content
    type(v2_t) :: roughness_z0, accumulated_precipitation, temperature_2m, humidity_2m, terrain, u_10m, v_10m, skin_temperature, &
                  surface_pressure, snow_water_equivalent, longwave_up, soil_totalmoisture, sensible_heat, temperature_2m_veg, &
                  temperature_2m_bare, mixing_ratio_2m_veg, mixing_ratio_2m_bare
    integer, pointer :: land_mask(:,:) => null(), veg_type(:,:) => null()
  end type
  type lsm_opt_t
    real :: max_swe
  end type
  type options_t
    type(lsm_opt_t) :: lsm_options
  end type
  type(domain_t), save :: dom
  type(options_t), save :: opt
@PARAMS@
  real, pointer, dimension(:,:) :: Z0, Ri, z_atm, lnz_atm_term, base_exchange_term, current_precipitation, windspd, CHS, CHS2, CQS2, QGH, &
                                   EMISS, QFX, QSFC, VEGFRAC
  double precision, pointer, dimension(:,:) :: RAINBL
  real :: DZS(4)
  integer :: num_soil_layers, ISICE, ISLAKE, exchange_term
  integer :: ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
contains
@CALC@
@SURFDIAG@
  subroutine s_init(domain)
    type(domain_t), intent(inout) :: domain
@Z0INIT@
@CURP0@
@CHS0@
@CHS20@
@RAINBL0@
@T2INIT@
@ZATM@
  end subroutine
  subroutine s_pre(domain)
    type(domain_t), intent(inout) :: domain
    integer :: i, j
@WINDSPD@
            if (exchange_term==1) then
@CALLCALC@
            endif
@CHSWIND@
@QGH@
@CURP@
  end subroutine
  subroutine s_post(domain, options)
    type(domain_t), intent(inout) :: domain
    type(options_t), intent(in) :: options
    integer :: i
@AFTER@
@SMSTOT@
@CALLDIAG@
  end subroutine

  subroutine ref_lnd_bind(nx, ny, its_, ite_, jts_, jte_, isice_, islake_, max_swe, p) bind(C, name="ref_lnd_bind")
    integer(c_int), value :: nx, ny, its_, ite_, jts_, jte_, isice_, islake_
    real(c_float), value :: max_swe
    type(c_ptr) :: p(*)
    ims = 1; ime = nx; jms = 1; jme = ny; kms = 1; kme = 2; kts = 1; kte = 2
    its = its_; ite = ite_; jts = jts_; jte = jte_
    ISICE = isice_; ISLAKE = islake_; exchange_term = 1; num_soil_layers = 4
    DZS = [0.1,0.3,0.6,1.0]
    opt%lsm_options%max_swe = max_swe
@BIND@
  end subroutine
  subroutine ref_lnd_init() bind(C, name="ref_lnd_init")
    call s_init(dom)
  end subroutine
  subroutine ref_lnd_pre() bind(C, name="ref_lnd_pre")
    call s_pre(dom)
  end subroutine
  subroutine ref_lnd_post() bind(C, name="ref_lnd_post")
    call s_post(dom, opt)
  end subroutine
end module
"""


def line(lsm, text, near, what):
    return excerpt(lsm, text, text, near, what)


def nth(lsm, start_text, near, last_text, count, what):
    """from the first line at or behind `near - 40` containing start_text to the count-th line behind it containing last_text"""
    a = next((n for n in range(max(0, near - 41), len(lsm)) if start_text in lsm[n]), None)
    assert a is not None and abs(a + 1 - near) <= 40, f"{what}: `{start_text}` not found near {near}"
    b, seen = a, 0
    while seen < count:
        b += 1
        seen += last_text in lsm[b]
    return "".join(lsm[a:b + 1])


def shim_text():
    lsm = open(os.path.join(REF, "src", "physics", "lsm_driver.f90")).readlines()
    parts = {
        "PARAMS": excerpt(lsm, "real, parameter :: SMALL_QV", "MIN_EXCHANGE_C", 87, "the parameters"),
        "CALC": excerpt(lsm, "subroutine calc_exchange_coefficient(wind,tskin,airt,exchange_C)", "end subroutine calc_exchange_coefficient", 244, "calc_exchange_coefficient"),
        "SURFDIAG": excerpt(lsm, "subroutine surface_diagnostics(HFX, QFX, TSK, QSFC, CHS2, CQS2,T2, Q2, PSFC, &", "end subroutine surface_diagnostics", 299, "surface_diagnostics"),
        "Z0INIT": line(lsm, "Z0 = domain%roughness_z0%data_2d", 566, ":566"),
        "CURP0": line(lsm, "current_precipitation = 0", 584, ":584"),
        "CHS0": line(lsm, "CHS = 0.01", 593, ":593"),
        "CHS20": line(lsm, "CHS2 = 0.01", 596, ":596"),
        "RAINBL0": line(lsm, "RAINBL = domain%accumulated_precipitation%data_2dd", 603, ":603"),
        "T2INIT": excerpt(lsm, "domain%temperature_2m%data_2d = domain%temperature%data_3d(:,kms,:)", "domain%humidity_2m%data_2d = domain%water_vapor%data_3d(:,kms,:)", 610, ":610-611"),
        "ZATM": excerpt(lsm, "z_atm = domain%z%data_3d(:,kts,:) - domain%terrain%data_2d", "endif", 992, ":992-997"),
        "WINDSPD": line(lsm, "windspd = sqrt(domain%u_10m%data_2d**2 + domain%v_10m%data_2d**2)", 1028, ":1028"),
        "CALLCALC": line(lsm, "call calc_exchange_coefficient(windspd,domain%skin_temperature%data_2d,domain%temperature%data_3d,CHS)", 1030, ":1030"),
        "CHSWIND": excerpt(lsm, "where(windspd<1) windspd=1", "CQS2 = CHS", 1144, ":1144-1147"),
        "QGH": nth(lsm, "do j=jms,jme", 1181, "enddo", 2, ":1181-1187"),
        "CURP": nth(lsm, "current_precipitation = (domain%accumulated_precipitation%data_2dd - RAINBL)", 1207, "", 0, ":1207"),
        "AFTER": nth(lsm, "where(domain%snow_water_equivalent%data_2d > options%lsm_options%max_swe)", 1280, "RAINBL = domain%accumulated_precipitation%data_2dd", 1, ":1280-1290"),
        "SMSTOT": nth(lsm, "domain%soil_totalmoisture%data_2d = domain%soil_water_content%data_3d(:,1,:) * DZS(1) * 1000", 1524, "enddo", 1, ":1524-1527"),
        "CALLDIAG": nth(lsm, "call surface_diagnostics(domain%sensible_heat%data_2d,", 1530, "domain%mixing_ratio_2m_bare%data_2d)", 1, ":1530-1545"),
    }
    assert "sat_mr(domain%temperature_2m%data_2d(i,j),domain%surface_pressure%data_2d(i,j))" in parts["QGH"]
    assert "longwave_up" in parts["AFTER"] and "lnz_atm_term=(karman/lnz_atm_term)**2" in parts["AFTER"] and parts["AFTER"].count("\n") <= 12
    bind, n = [], 0
    for _, target in BIND2:
        n += 1; bind.append(f"    call c_f_pointer(p({n}), {target}, [nx,ny])")
    for _, target in BIND2D:
        n += 1; bind.append(f"    call c_f_pointer(p({n}), {target}, [nx,ny])")
    for _, target in BIND2I:
        n += 1; bind.append(f"    call c_f_pointer(p({n}), {target}, [nx,ny])")
    for _, target, nz in BIND3:
        n += 1; bind.append(f"    call c_f_pointer(p({n}), {target}, [nx,{nz},ny])")
    parts["BIND"] = "\n".join(bind)
    text = SHIM
    for k, v in parts.items():
        text = text.replace("@" + k + "@", v)
    return text


def build_reference(tmp):
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-fcoarray", "-w", "-DUSE_ASSERTIONS=.false.", "-I" + os.path.join(src, "physics"), "-I" + os.path.join(src, "utilities")]
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    run([FC, "-c", "-O2", "-fPIC", "-w", os.path.join(ROOT, "oracle", "ref_link_stubs.f90"), "-o", "ref_link_stubs.o"])
    run(["gcc", "-c", "-fPIC", os.path.join(ROOT, "oracle", "ref_link_stubs.c"), "-o", "ref_link_stubs_c.o"])
    objs = ["ref_link_stubs.o", "ref_link_stubs_c.o"]
    for m in MODULES + ["physics/lsm_noahlsm", "physics/lsm_noahdrv"]:
        o = os.path.basename(m) + ".o"
        run([FC] + flags + [os.path.join(src, m + ".f90"), "-o", o])
        objs.append(o)
    open(os.path.join(tmp, "noah_shim.f90"), "w").write(G.SHIM % dict(args=G.wrap(G.REF3 + G.REF2 + G.REFS), a3=G.wrap(G.REF3), a2=G.wrap(G.REF2),
                                                                     **{"as": G.wrap(G.REFS)}))
    open(os.path.join(tmp, "lnd_shim.f90"), "w").write(shim_text())
    for s in ("noah_shim", "lnd_shim"):
        run([FC] + flags + [s + ".f90", "-o", s + ".o"])
        objs.append(s + ".o")
    und = subprocess.check_output(["nm", "-u"] + objs, cwd=tmp, text=True)
    dfn = subprocess.check_output(["nm", "--defined-only"] + objs, cwd=tmp, text=True)
    undef = {l.split()[1] for l in und.splitlines() if len(l.split()) == 2 and l.split()[0] == "U" and l.split()[1].startswith("_QM")}
    defined = {l.split()[2] for l in dfn.splitlines() if len(l.split()) == 3}
    open(os.path.join(tmp, "defsyms.rsp"), "w").write("\n".join(f"-Wl,--defsym,{s}=0" for s in sorted(undef - defined)))
    run([FC, "-shared", "-o", "liblndref.so"] + objs + ["@defsyms.rsp"])
    for t in ("VEGPARM.TBL", "SOILPARM.TBL", "GENPARM.TBL"):
        shutil.copy(os.path.join(REF, "run", t), tmp)
    return ctypes.CDLL(os.path.join(tmp, "liblndref.so"))


def bind(L, c, R, n):
    """the shim's pointers onto the reference-side state R and the forcing of call n; returns what must outlive the calls"""
    F = c["forcing"][max(n, 0)]                                                      # n < 0: lsm_init, ahead of the first call
    s2 = (c["ny"], c["nx"])
    two = lambda a, b: np.ascontiguousarray(np.stack([a, b], axis=1))
    B = dict(R)
    B.update(terrain=c["terrain"], u10=F["u10"], v10=F["v10"], psfc=F["psfc"], precip=F["precip"], vegfra=c["vegfra"], ivgtyp=c["ivgtyp"],
             land_mask=np.ascontiguousarray(c["xland"], np.int32), t2veg=np.zeros(s2, f32), windspd=np.full(s2, 3.0, f32),
             t3=two(F["t"], F["t"]), qv3=two(F["qv"], F["qv"]), z3=two(c["z1"], c["z1"] + f32(80.0)))
    if n < 0:
        B["precip"] = c["precip0"]
    names = [k for k, _ in BIND2] + [k for k, _ in BIND2D] + [k for k, _ in BIND2I] + [k for k, _, _ in BIND3]
    for k in names:
        want = f64 if k in ("precip", "rainbl8") else np.int32 if k in ("land_mask", "ivgtyp") else f32
        assert B[k].dtype == want and B[k].flags.c_contiguous, k
    ptr = (ctypes.c_void_p * len(names))(*[B[k].ctypes.data for k in names])
    its, ite, jts, jte = LN.tile_of(c)
    ci = ctypes.c_int
    L.ref_lnd_bind(ci(c["nx"]), ci(c["ny"]), ci(its), ci(ite), ci(jts), ci(jte), ci(N.ISICE), ci(N.ISLAKE), ctypes.c_float(float(c["max_swe"])), ptr)
    return B, ptr


def compare(what, R, O, keys, where=None):
    bad = {}
    for k in keys:
        a, b = (R[k], O[k]) if where is None else (R[k][where], O[k][where])
        d = LN.bitdiff(a, b)
        if d:
            bad[k] = d
    if bad:
        print("  ", what, "differing bits:", bad)
    return not bad


def make(L, tmp, tab, name, p, write, cover):
    c = LN.make_case(tab, **p)
    nc = c["noah_case"]
    its, ite, jts, jte = LN.tile_of(c)
    rows, cols = np.arange(jts - 1, jte), np.arange(its - 1, ite)
    tile = (slice(jts - 1, jte), slice(None), slice(its - 1, ite))
    tile2 = (slice(jts - 1, jte), slice(its - 1, ite))
    R, O, Ofma = LN.state0(c), LN.state0(c), LN.state0(c)
    out = {"input_fingerprint": np.float64(LN.fingerprint(c))}
    # lsm_init: LSM_NOAH_INIT on the grid's tile, then the statements of the coupling
    S = G.ref_init(L, tmp, nc, R, rows, cols)
    for k in ("sh2o", "snoalb", "snowh", "canwat"):
        R[k][tile if R[k].ndim == 3 else tile2] = S[k]
    B, ptr = bind(L, c, R, -1)
    L.ref_lnd_init()
    LN.lsm_init(tab, c, O)
    LN.lsm_init(tab, c, Ofma, LN.lib(contract=True))
    ok = compare(f"{name} lsm_init", R, O, LN.INIT)
    ok = compare(f"{name} LSM_NOAH_INIT (tile)", {k: R[k][tile if R[k].ndim == 3 else tile2] for k in ("sh2o", "snoalb", "snowh", "canwat")},
                 {k: O[k][tile if O[k].ndim == 3 else tile2] for k in ("sh2o", "snoalb", "snowh", "canwat")}, ("sh2o", "snoalb", "snowh", "canwat")) and ok
    for k in LN.INIT + ["sh2o", "snoalb", "snowh", "canwat"]:
        assert np.isfinite(R[k]).all(), (name, k)
        out["init_" + k] = R[k].copy()
    ice = N.ice_cells(c)
    share_ice = float(ice.mean())
    assert share_ice > 0 and (cover is None or share_ice <= 0.05), f"{name}: land ice is {share_ice:.3f} of the cells (a fixture: at most 0.05)"
    gates, flags, fma_differs = [], [], False
    for n in range(len(c["forcing"])):
        now = c["clock"][n]
        r_open, r_dt = LN.gate(c, R, now)
        o_open, o_dt = LN.gate(c, O, now)
        LN.gate(c, Ofma, now)
        assert r_open == o_open and r_dt == o_dt
        gates.append(bool(r_open))
        if r_open:
            B, ptr = bind(L, c, R, n)
            L.ref_lnd_pre()
            pf = LN.pre(c, O, n)
            LN.pre(c, Ofma, n, LN.lib(contract=True))
            ok = compare(f"{name} call {n + 1} ahead of lsm_noah", R, O, ["rib", "chs", "chs2", "cqs2", "qgh", "rainbl_step"]) and ok
            S = G.ref_call(L, dict(nc, dt=f32(r_dt)), R, n, rows, cols)
            N.lsm_noah(tab, nc, O, n, (its, ite, jts, jte), r_dt)
            N.lsm_noah(tab, nc, Ofma, n, (its, ite, jts, jte), r_dt)
            for k in N.OUT:
                R[k][tile if R[k].ndim == 3 else tile2] = S[k]
            for k in N.ICE_UNSET:                                                  # (LAND ICE above)
                R[k][ice] = O[k][ice]
            B, ptr = bind(L, c, R, n)
            L.ref_lnd_post()
            qf = LN.post(c, O, n)
            LN.post(c, Ofma, n, None, LN.lib(contract=True))
            flags.append((pf, qf))
        # lsm_noah's outputs on its tile (outside it the reference's LSM_NOAH_INIT has not run: make_golden_noah.py), the whole-array statements everywhere
        ok = compare(f"{name} call {n + 1} (tile)", {k: R[k][tile if R[k].ndim == 3 else tile2] for k in N.OUT},
                     {k: O[k][tile if O[k].ndim == 3 else tile2] for k in N.OUT}, N.OUT) and ok
        ok = compare(f"{name} call {n + 1}", R, O, LN.DRV + LN.WHOLE) and ok
        fma_differs = fma_differs or any(LN.bitdiff(R[k], Ofma[k]) for k in LN.DRV)
        for k in N.OUT + LN.DRV:
            assert np.isfinite(R[k]).all(), f"(1) {name}: the reference's {k} is not finite after call {n + 1}"
            out[f"call{n + 1}_{k}"] = R[k].copy()
    assert gates.count(False) == 1 and gates[0], f"(2) {name}: gates {gates}"
    sh = LN.shares(c, flags)
    assert sh["wind0"] >= 1, f"(2) {name}: no cell of the tile has wind == 0"
    if cover is not None:
        cover[name] = sh
    print(name, "restatement == reference:", ok, " gates", gates, f" land ice {share_ice:.3f} of the cells", " FMA-contracted restatement differs:", fma_differs)
    if write and ok:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), shares=np.array(json.dumps(sh)), gates=np.array(gates),
                            fma_contracted_differs=np.array(fma_differs), **out)
    return ok, fma_differs


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_lsm_noah: the reference sources are not present")
    write = "--dry" not in sys.argv
    with tempfile.TemporaryDirectory(prefix="icar_lndref_") as tmp:
        L = build_reference(tmp)
        first = N.make_case({"maxsmc": np.full(N.NSLTYPE, 0.4), "wltsmc": np.full(N.NSLTYPE, 0.1)}, nx=5, ny=4, seed=99, dt=600.0, t=[280.0], sw=[100],
                            pr=[(0.5, 1.0)], snow0=0.2)
        G.ref_init(L, tmp, first, N.state0(first))                                    # reads the three tables
        tab = G.tables(L)
        stored = N.load_tables()
        assert all(np.array_equal(np.asarray(tab[k]), np.asarray(stored[k])) for k in stored), "the tables differ from tests/golden/noah_tables.npz"
        cover = {}
        res = [make(L, tmp, tab, n, p, False, cover) for n, p in LN.CASES.items()]
        res += [make(L, tmp, tab, n, p, False, None) for n, p in LN.SEEDS.items()]
        good = all(ok for ok, _ in res)
        for k in LN.REQUIRED + LN.NOT_REACHED:
            best = max(cover, key=lambda name: cover[name][k])
            print(f"  coverage {k:12s} best share {cover[best][k]:.3f} ({best})")
            if k in LN.REQUIRED and cover[best][k] < 0.02:
                good = False
                print("    NOT MET")
            if k in LN.NOT_REACHED and cover[best][k] > 0:
                good = False
                print("    REACHED: move it to REQUIRED")
        print("  the FMA-contracted restatement differs from the reference in some case:", any(f for _, f in res))
        if good and write:
            for n, p in LN.CASES.items():
                make(L, tmp, tab, n, p, True, None)
        sys.exit(0 if good else 1)

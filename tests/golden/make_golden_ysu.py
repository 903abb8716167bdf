#!/usr/bin/env python
"""Golden vectors of the boundary-layer slot with boundarylayer = kPBL_YSU under tests/golden/ysu_*.npz made by RUNNING THE REFERENCE'S
OWN CODE, compiled with the flang of oracle/build_ref.sh in a temporary directory outside the repository.

How each range is pinned:
  ysu, ysu2d, tridin, ysuinit        src/physics/pbl_ysu.f90 WHOLE and unmodified
  da_sfc_wtq, da_tp_to_qs            src/utilities/pbl_utilities.f90 WHOLE and unmodified, both with src/constants/icar_constants.f90 and
                                     wrf_constants.f90
  pbl_init's YSU branch              src/physics/pbl_driver.f90: the statements from `allocate(windspd(` to the end of the call of
                                     ysuinit (:132-193)
  pbl's YSU branch                   the wind speed with its floor, calc_Richardson_nr and the call of da_sfc_wtq (:227-254), the call
                                     of ysu with its argument expressions (:257-323), the four updates and the six resets (:343-354)
  calc_Richardson_nr                 src/utilities/atm_utilities.f90:1131-1139
all EXCERPTED BY THEIR TEXT at generation time into a shim module whose domain_t holds pointer arrays under the reference's member
names (pbl_driver.f90 as a whole uses a live domain_t with coarray members).  The ranges are found by their text; the line numbers
quoted are only checked to lie within 40 lines.

Every case of tests/ysu_oracle.py:CASES runs CALLS carried calls with growing dt; between calls domain%temperature is made again from
the potential temperature as diagnostic_update does.  Stored: pbl_init's arrays, after every call the 2-D results, exch_h and the four
scalar tendencies as ysu leaves them in full, SHA-256 of the two wind tendencies and of the four updated fields; after the last call
the wind tendencies and cloud water in full.  The generator REFUSES TO WRITE unless tests/support/ysu_oracle.c -- with the forms of
** that icar_amd/csrc/ysu_column.h states -- reproduces the compiled reference bit for bit on every case and on the two further seeds
of EXTRA_SEEDS (checked, not stored), every result is finite, ustar is positive everywhere (see ysu_column.h on use_ust_wrf) and the
coverage conditions of tests/test_ysu_oracle.py hold.  Only runs where the reference is present."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ysu_oracle as Y  # noqa: E402

REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402

SHIM = """
module ysu_shim
  use iso_c_binding
  use icar_constants
  use mod_wrf_constants, only : EOMEG
  use module_bl_ysu, only : ysuinit, ysu
  use mod_pbl_utilities, only : da_sfc_wtq
  implicit none
  type v3_t
    real, pointer :: data_3d(:,:,:) => null()
  end type
  type v2_t
    real, pointer :: data_2d(:,:) => null()
  end type
  type tend_t
    real, pointer, dimension(:,:,:) :: u => null(), v => null(), th_pbl => null(), qv_pbl => null(), qc_pbl => null(), qi_pbl => null()
  end type
  type domain_t
    type(v3_t) :: z, temperature, pressure, cloud_water_mass, u_mass, v_mass, potential_temperature, water_vapor, cloud_ice_mass, &
                  pressure_interface, exner, dz_interface, coeff_heat_exchange_3d
    type(v2_t) :: terrain, roughness_z0, u_10m, v_10m, skin_temperature, surface_pressure, ground_surf_temperature, sensible_heat, &
                  latent_heat, hpbl
    type(tend_t) :: tend
    real, pointer :: ustar(:,:) => null(), znu(:) => null(), znw(:) => null()
    integer, pointer :: kpbl(:,:) => null(), land_mask(:,:) => null()
    real :: dx
  end type
  type(domain_t), save :: dom
  ! the module variables of the driver that the excerpts below name, declared for this shim
  real, allocatable :: windspd(:,:), Ri(:,:), z_atm(:,:), zol(:,:), hol(:,:), psim(:,:), psih(:,:), gz1oz0(:,:), xland_real(:,:), regime(:,:)
  real, allocatable :: u10d(:,:), v10d(:,:), t2d(:,:), q2d(:,:)
  real, allocatable :: tend_u_ugrid(:,:,:), tend_v_vgrid(:,:,:)
  integer :: ims, ime, jms, jme, kms, kme
  integer :: its, ite, jts, jte, kts, kte
  integer :: ids, ide, jds, jde, kds, kde
  integer :: i, j, k
  logical :: restart, allowed_to_read, flag_qi
  real, allocatable, target :: znu_store(:), znw_store(:)
contains
@RICHARDSON@

  subroutine init_body(domain)
    type(domain_t), intent(inout) :: domain
    allowed_to_read = .True.
    restart = .False.
    flag_qi = .true.
@INIT@
  end subroutine

  subroutine sfc_body(domain)
    type(domain_t), intent(inout) :: domain
@SFC@
  end subroutine

  subroutine ysu_body(domain, dt_in)
    type(domain_t), intent(inout) :: domain
    real, intent(in) :: dt_in
@YSU@
  end subroutine

  subroutine apply_body(domain, dt_in)
    type(domain_t), intent(inout) :: domain
    real, intent(in) :: dt_in
@APPLY@
  end subroutine

  subroutine ref_ysu_bind(nx, nz, ny, its_, ite_, jts_, jte_, dx, z, terrain, z0, land_mask, t, p, qc, um, vm, th, qv, qi, pint, pii, dz, exch, &
                          u10, v10, tsk, psfc, tg, hfx, lh, hpbl_, ustar, kpbl, tu, tv, tth, tqv, tqc, tqi) bind(C, name="ref_ysu_bind")
    integer(c_int), value :: nx, nz, ny, its_, ite_, jts_, jte_
    real(c_float), value :: dx
    real(c_float), dimension(nx,nz,ny), target :: z, t, p, qc, um, vm, th, qv, qi, pint, pii, dz, exch, tu, tv, tth, tqv, tqc, tqi
    real(c_float), dimension(nx,ny), target :: terrain, z0, u10, v10, tsk, psfc, tg, hfx, lh, hpbl_, ustar
    integer(c_int), dimension(nx,ny), target :: land_mask, kpbl
    ims = 1; ime = nx; kms = 1; kme = nz; jms = 1; jme = ny
    ids = 1; ide = nx + 1; kds = 1; kde = nz + 1; jds = 1; jde = ny + 1
    its = its_; ite = ite_; jts = jts_; jte = jte_; kts = 1; kte = nz
    if (allocated(windspd)) deallocate(windspd, Ri, z_atm, zol, hol, psim, psih, u10d, v10d, t2d, q2d, gz1oz0, xland_real, regime, &
                                       tend_u_ugrid, tend_v_vgrid, znu_store, znw_store)
    allocate(znu_store(kms:kme)); allocate(znw_store(kms:kme)); znu_store = 0; znw_store = 0
    dom%dx = dx; dom%znu => znu_store; dom%znw => znw_store
    dom%z%data_3d => z; dom%temperature%data_3d => t; dom%pressure%data_3d => p; dom%cloud_water_mass%data_3d => qc
    dom%u_mass%data_3d => um; dom%v_mass%data_3d => vm; dom%potential_temperature%data_3d => th; dom%water_vapor%data_3d => qv
    dom%cloud_ice_mass%data_3d => qi; dom%pressure_interface%data_3d => pint; dom%exner%data_3d => pii; dom%dz_interface%data_3d => dz
    dom%coeff_heat_exchange_3d%data_3d => exch
    dom%terrain%data_2d => terrain; dom%roughness_z0%data_2d => z0; dom%u_10m%data_2d => u10; dom%v_10m%data_2d => v10
    dom%skin_temperature%data_2d => tsk; dom%surface_pressure%data_2d => psfc; dom%ground_surf_temperature%data_2d => tg
    dom%sensible_heat%data_2d => hfx; dom%latent_heat%data_2d => lh; dom%hpbl%data_2d => hpbl_
    dom%ustar => ustar; dom%kpbl => kpbl; dom%land_mask => land_mask
    dom%tend%u => tu; dom%tend%v => tv; dom%tend%th_pbl => tth; dom%tend%qv_pbl => tqv; dom%tend%qc_pbl => tqc; dom%tend%qi_pbl => tqi
    call init_body(dom)
  end subroutine

  subroutine ref_ysu_temperature(nx, nz, ny, t) bind(C, name="ref_ysu_temperature")
    integer(c_int), value :: nx, nz, ny
    real(c_float), dimension(nx,nz,ny), target :: t
    dom%temperature%data_3d => t
  end subroutine

  subroutine ref_ysu_sfc() bind(C, name="ref_ysu_sfc")
    call sfc_body(dom)
  end subroutine

  subroutine ref_ysu_ysu(dt) bind(C, name="ref_ysu_ysu")
    real(c_float), value :: dt
    call ysu_body(dom, dt)
  end subroutine

  subroutine ref_ysu_apply(dt) bind(C, name="ref_ysu_apply")
    real(c_float), value :: dt
    call apply_body(dom, dt)
  end subroutine

  subroutine ref_ysu_get(nx, ny, which, out) bind(C, name="ref_ysu_get")
    integer(c_int), value :: nx, ny, which
    real(c_float), dimension(nx,ny) :: out
    select case (which)
    case (0); out = z_atm
    case (1); out = gz1oz0
    case (2); out = zol
    case (3); out = hol
    case (4); out = windspd
    case (5); out = Ri
    case (6); out = psim
    case (7); out = psih
    case (8); out = regime
    case (9); out = xland_real
    end select
  end subroutine
end module
"""
GET = {"z_atm": 0, "gz1oz0": 1, "zol": 2, "hol": 3, "windspd": 4, "ri": 5, "psim": 6, "psih": 7, "regime": 8, "xland_real": 9}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def excerpt(lines, first, last, near, what, start=0):
    a = next((n for n in range(start, len(lines)) if first in lines[n]), None)
    assert a is not None, f"{what}: `{first}` not found in the reference"
    b = next((n for n in range(a, len(lines)) if last in lines[n]), None)
    assert b is not None, f"{what}: `{last}` not found behind it"
    assert abs(a + 1 - near) <= 40, f"{what}: found at line {a + 1}, expected near {near}"
    return "".join(lines[a:b + 1]), b


def shim_text():
    drv = open(os.path.join(REF, "src", "physics", "pbl_driver.f90")).readlines()
    atm = open(os.path.join(REF, "src", "utilities", "atm_utilities.f90")).readlines()
    ini0 = next(n for n, l in enumerate(drv) if l.lstrip().startswith("subroutine pbl_init("))
    init, _ = excerpt(drv, "allocate(windspd(ims:ime, jms:jme))", ",kts=kts, kte=kte-1)", 132, "pbl_init's YSU branch", ini0)
    assert "z_atm = domain%z%data_3d(:,kts,:) - domain%terrain%data_2d" in init and "gz1oz0 = log(z_atm / domain%roughness_z0%data_2d)" in init
    assert "zol = 10" in init and "hol = 1000.0" in init and "xland_real=real(domain%land_mask)" in init and "call ysuinit(" in init
    pbl0 = next(n for n, l in enumerate(drv) if l.lstrip().startswith("subroutine pbl("))
    sfc, s_end = excerpt(drv, "windspd = sqrt(domain%u_10m%data_2d**2 + domain%v_10m%data_2d**2)", ",ims=ims, ime=ime, jms=jms, jme=jme)", 227,
                         "the surface-layer statements", pbl0)
    assert "where(windspd==0) windspd=1e-5" in sfc and "call calc_Richardson_nr(Ri,domain%temperature%data_3d, domain%skin_temperature%data_2d, z_atm, windspd)" in sfc
    assert "qs=domain%cloud_water_mass%data_3d(:,1,:)" in sfc and "tg=domain%ground_surf_temperature%data_2d" in sfc
    assert "qfx=domain%latent_heat%data_2d/LH_vaporization" in sfc and "ust_wrf=domain%ustar" in sfc
    ysu, y_end = excerpt(drv, "call ysu(u3d=domain%u_mass%data_3d", ",regime=regime", 257, "the call of ysu", s_end)
    assert ",kts=kts, kte=kte-1" in ysu and ",tsk=domain%skin_temperature%data_2d" in ysu and ",wspd=windspd" in ysu and "mut=" in ysu
    assert all(l.lstrip().startswith("!") for l in ysu.splitlines() if "mut=" in l or "p_top=" in l), "mut / p_top are passed after all"
    app, _ = excerpt(drv, "domain%water_vapor%data_3d            =  domain%water_vapor%data_3d            + domain%tend%qv_pbl  * dt_in",
                     "domain%tend%v         = 0", 343, "the updates and resets", y_end)
    assert app.count("* dt_in") == 4 and app.count("= 0") == 6
    ric, _ = excerpt(atm, "subroutine calc_Richardson_nr(Ri,airt_3d, tskin, z_atm, wind_2d)", "end subroutine calc_Richardson_nr", 1131,
                     "calc_Richardson_nr")
    assert "Ri = gravity/airt_3d(:,1,:) * (airt_3d(:,1,:)-tskin)*z_atm/(wind_2d**2)" in ric
    return SHIM.replace("@RICHARDSON@", ric).replace("@INIT@", init).replace("@SFC@", sfc).replace("@YSU@", ysu).replace("@APPLY@", app)


def build_reference(tmp):
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-w"]
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    objs = []
    for f in (os.path.join(src, "constants", "icar_constants.f90"), os.path.join(src, "constants", "wrf_constants.f90"),
              os.path.join(src, "physics", "pbl_ysu.f90"), os.path.join(src, "utilities", "pbl_utilities.f90")):
        o = os.path.basename(f)[:-4] + ".o"
        run([FC] + flags + [f, "-o", o]); objs.append(o)
    open(os.path.join(tmp, "ysu_shim.f90"), "w").write(shim_text())
    try:
        run([FC] + flags + ["ysu_shim.f90", "-o", "ysu_shim.o"]); objs.append("ysu_shim.o")
    except subprocess.CalledProcessError as e:
        sys.exit("make_golden_ysu: the shim does not compile:\n" + e.stderr.decode()[-4000:])
    run([FC, "-shared", "-o", "libysuref.so"] + objs)
    # which form each ** of ysu2d and da_sfc_wtq took: read off the reference's LLVM IR (DESIGN 3.3 quotes the list)
    forms = {}
    for f, name in ((os.path.join(src, "physics", "pbl_ysu.f90"), "pbl_ysu"), (os.path.join(src, "utilities", "pbl_utilities.f90"), "pbl_utilities")):
        run([FC, "-S", "-emit-llvm", "-cpp", "-O2", "-fPIC", "-w", f, "-o", name + ".ll"])
        ir = open(os.path.join(tmp, name + ".ll")).read().splitlines()
        forms[name] = sorted(l.split("float ")[-1].rstrip(")") for l in ir if "@llvm.pow.f32" in l and "call" in l)
    return ctypes.CDLL(os.path.join(tmp, "libysuref.so")), forms


# the exponents that stay calls of powf, as icar_amd/csrc/ysu_column.h states them (LLVM prints a float constant as the double it equals)
EXPECTED_POW = {"pbl_ysu": sorted(["-2.500000e-01", "-5.000000e-01", "0x3FD5555560000000", "4.000000e+00", "0xBFC70A3D80000000", "0x3FE5555560000000",
                                   "0x3FD5555560000000"]),
                "pbl_utilities": sorted(["0x3FD51EB860000000", "0x3FD22763C0000000", "0x3FD22763C0000000", "0x3FD51EB860000000", "2.500000e-01",
                                         "2.500000e-01", "2.500000e-01", "0xBFE3333340000000", "0x3FD22763C0000000"])}

_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def ref_get(L, c, name):
    ny, nz, nx = c["z"].shape
    out = np.zeros((ny, nx), np.float32)
    L.ref_ysu_get(ctypes.c_int(nx), ctypes.c_int(ny), ctypes.c_int(GET[name]), _p(out))
    return out


def ref_bind(L, c, A, tile=None):
    ny, nz, nx = c["z"].shape
    its, ite, jts, jte = tile or Y.tile_of(c)
    ci = ctypes.c_int
    L.ref_ysu_bind(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ctypes.c_float(float(c["dx"])), _p(c["z"]), _p(c["terrain"]),
                   _p(c["roughness_z0"]), _p(c["land_mask"]), _p(A["temperature"]), _p(c["pressure"]), _p(A["cloud_water"]), _p(c["u_mass"]),
                   _p(c["v_mass"]), _p(A["potential_temperature"]), _p(A["water_vapor"]), _p(A["cloud_ice"]), _p(c["pressure_interface"]),
                   _p(c["exner"]), _p(c["dz_interface"]), _p(A["exch_h"]), _p(c["u_10m"]), _p(c["v_10m"]), _p(c["skin_temperature"]),
                   _p(c["surface_pressure"]), _p(c["ground_surf_temperature"]), _p(c["sensible_heat"]), _p(c["latent_heat"]), _p(A["hpbl"]),
                   _p(c["ustar"]), _p(A["kpbl"]), _p(A["tend_u"]), _p(A["tend_v"]), _p(A["tend_th"]), _p(A["tend_qv"]), _p(A["tend_qc"]), _p(A["tend_qi"]))
    for k in Y.INIT2:
        A[k] = ref_get(L, c, k)


def ref_call(L, c, A, n, keep):
    ny, nz, nx = c["z"].shape
    if n:
        Y.rediagnose(c, A)
        L.ref_ysu_temperature(ctypes.c_int(nx), ctypes.c_int(nz), ctypes.c_int(ny), _p(A["temperature"]))
    L.ref_ysu_sfc()
    for k in ("windspd", "ri", "psim", "psih", "regime"):
        A[k] = ref_get(L, c, k)
    L.ref_ysu_ysu(ctypes.c_float(Y.DT[n]))
    A["hol"] = ref_get(L, c, "hol")
    keep.update({k: A[k].copy() for k in Y.TEND})
    L.ref_ysu_apply(ctypes.c_float(Y.DT[n]))


COMPARED = Y.STATE3 + Y.TEND + ["exch_h"] + Y.OUT2 + ["z_atm", "gz1oz0", "zol"]


def make(L, name, p):
    c = Y.make_case(**p)
    assert (c["ustar"] > 0).all(), f"{name}: ustar <= 0 somewhere (da_sfc_wtq's SAVEd use_ust_wrf makes such a cell depend on the one before it)"
    A = Y.state(c)
    # what the reference never writes must not differ by accident: poison nothing, both start from the same zeros
    ref_bind(L, c, A)
    O = Y.state(c)
    same = not any(Y.bitdiff(A[k], O[k]) for k in Y.INIT2)
    out = {"input_fingerprint": np.float64(Y.fingerprint(c))}
    for k in Y.INIT2:
        out["init_" + k] = A[k].copy()
    covs = []
    for n in range(Y.CALLS):
        keepA, keepO = {}, {}
        ref_call(L, c, A, n, keepA)
        Y.run_oracle(c, O, n, keep=keepO)
        d = {k: Y.bitdiff(A[k], O[k]) for k in COMPARED if k not in Y.TEND}
        d.update({k: Y.bitdiff(keepA[k], keepO[k]) for k in Y.TEND})
        same = same and not any(d.values())
        if any(d.values()): print("   call", n + 1, "differing bits:", {k: v for k, v in d.items() if v})
        for k in Y.STATE3 + ["exch_h", "hpbl", "hol", "psim", "psih", "regime", "ri", "windspd"]:
            assert np.isfinite(A[k]).all(), f"{name}: the reference's {k} is not finite after call {n + 1}"
        for k in Y.TEND:
            assert np.isfinite(keepA[k]).all(), f"{name}: the reference's {k} is not finite in call {n + 1}"
            assert not A[k].any(), f"{name}: {k} is not zero behind the reset"
        assert any(keepA[k].any() for k in ("tend_th", "tend_qv")), f"{name}: nothing mixes"
        for k in Y.OUT2 + ["exch_h"]:
            out[f"call{n + 1}_{k}"] = A[k].copy()
        for k in ("tend_th", "tend_qv", "tend_qc", "tend_qi"):
            out[f"call{n + 1}_{k}"] = keepA[k].copy()
        for k in ("tend_u", "tend_v"):
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(keepA[k]))
        for k in Y.STATE3:
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(A[k]))
        covs.append(Y.coverage(c, A, keepO))
    for k in ("tend_u", "tend_v"):
        out[f"call{Y.CALLS}_{k}"] = keepA[k].copy()
    out[f"call{Y.CALLS}_cloud_water"] = A["cloud_water"].copy()
    floor = float((A["windspd"] == np.float32(1e-5)).mean())
    print(name, "restatement == reference:", same, "| 1e-5 floor in", round(floor, 3), "of the cells | water", round(float((c["land_mask"] == 2).mean()), 3))
    return same, out, covs, floor, c


def holds(covs, floors, cases):
    """the coverage conditions over all fixtures: each must hold in some fixture (tests/test_ysu_oracle.py recomputes them)"""
    best = lambda k: max(cv[k] for cv in covs)
    two_sided = lambda k: any(0.01 <= cv[k] <= 0.99 for cv in covs)
    bad = []
    if not any(cv["unstable"] >= 0.2 and cv["stable"] >= 0.2 for cv in covs): bad.append("unstable and stable columns >= 20 % each")
    for r in (1, 2, 3, 4):
        if best(f"regime{r}") < 0.02: bad.append(f"regime {r} in >= 2 % ({best(f'regime{r}'):.4f})")
    if best("kpbl_distinct_with_pblflg") < 4: bad.append("kpbl with pblflg: >= 4 distinct values")
    if best("kpbl_is_1") < 0.05: bad.append("kpbl = 1 in >= 5 %")
    for k in ("moist", "ri_neg", "entrain", "xkzmin", "xkzmax", "prmax", "gamcrt", "gamcrq", "rimin"):
        if not two_sided(k): bad.append(f"{k} taken and not taken in >= 1 % (best share {best(k):.4f})")
    # prmin cannot be taken: below the boundary-layer top prnum >= phih/phim + bfac karman sfcfrac > 0.2788, above it prnum >= 1
    if best("prmin") != 0.0: bad.append("prmin was taken although the arithmetic excludes it")
    if max(floors) < 0.01: bad.append("the 1e-5 floor of the wind speed in >= 1 % of a fixture's cells")
    if not any((c["land_mask"] == 1).all() for c in cases): bad.append("an all-land fixture")
    if not any((c["land_mask"] == 2).mean() >= 0.3 for c in cases): bad.append("a fixture with >= 30 % water")
    return bad


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_ysu: the reference sources are not present")
    write = "--dry" not in sys.argv
    with tempfile.TemporaryDirectory(prefix="icar_ysuref_") as tmp:
        L, forms = build_reference(tmp)
        print("powf calls the compiled reference keeps (exponents):", json.dumps(forms))
        assert forms == EXPECTED_POW, "the compiled reference keeps other powers as calls than ysu_column.h states"
        res = {n: make(L, n, p) for n, p in Y.CASES.items()}
        extra = {n: make(L, n, p) for n, p in Y.EXTRA_SEEDS.items()}
        ok = all(r[0] for r in res.values()) and all(r[0] for r in extra.values())
        covs = [cv for r in res.values() for cv in r[2]]
        bad = holds(covs, [r[3] for r in res.values()], [r[4] for r in res.values()])
        for b in bad: print("coverage condition not met:", b)
        if write and ok and not bad:
            for n, (same, out, cv, floor, c) in res.items():
                path = os.path.join(HERE, n + ".npz")
                np.savez_compressed(path, params=np.array(json.dumps(Y.CASES[n])), coverage=np.array(json.dumps(cv)), **out)
                print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")
        elif write:
            print("NOTHING WRITTEN")
        sys.exit(0 if ok and not bad else 1)

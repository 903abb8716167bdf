#!/usr/bin/env python
"""Golden vectors of the convection slot under tests/golden/cu_bmj_*.npz made by RUNNING THE REFERENCE'S OWN CODE, compiled with the
flang of oracle/build_ref.sh in a temporary directory outside the repository.

How each range is pinned:
  BMJINIT, BMJDRV, BMJ, TTBLEX, SPLINE   src/physics/cu_bmj.f90 WHOLE with src/constants/wrf_constants.f90 and icar_constants.f90, from a
                          temporary copy in which the PRIVATE attribute of the table declarations is removed so that the shim can read
                          the tables.  The generator asserts that exactly those declaration lines differ from the original.
  convect's statements    src/physics/cu_driver.f90: the zeroing loop (`do j=jts,jte` .. `enddo`, :272-282), the call of BMJDRV
                          (:434-465) and the tendency / precipitation loop (:483-500), EXCERPTED BY THEIR TEXT at generation time into
                          a shim module whose domain_t / options_t hold pointer arrays and scalars under the reference's member names;
                          cu_driver.f90 as a whole uses Tiedtke, NSAS and a live domain_t with coarray members.
  init_convection         XLAND (:139-140), lowlyr, kpbl and the BMJINIT call (:230-243) are restated in the shim (four statements).
The ranges are found by their text; the line numbers quoted are only checked to lie within 40 lines.

Every case of tests/bmj_oracle.py:CASES runs CALLS carried calls with growing dt; between calls domain%temperature is made again from
the potential temperature as diagnostic_update does.  Stored: the 2-D results and the two tendencies in full after every call, SHA-256
of the four updated 3-D fields after every call and those fields in full after the last.  The generator asserts that
tests/support/bmj_oracle.c reproduces the compiled reference bit for bit before it writes anything.  Only runs where the reference is
present; tests/test_bmj_oracle.py pins the restatement to these files everywhere."""
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
import bmj_oracle as B  # noqa: E402

REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402

SHIM = """
module cu_shim
  use iso_c_binding
  use icar_constants
  use mod_wrf_constants
  use module_cu_bmj
  implicit none
  type v3_t
    real, pointer :: data_3d(:,:,:) => null()
  end type
  type v2_t
    real, pointer :: data_2d(:,:) => null()
  end type
  type v2d_t
    real(c_double), pointer :: data_2dd(:,:) => null()
  end type
  type tend_t
    real, pointer, dimension(:,:,:) :: qv => null(), th => null(), qc => null(), qi => null(), qs => null(), qr => null(), u => null(), v => null()
  end type
  type domain_t
    type(v3_t) :: potential_temperature, temperature, density, dz_interface, pressure_interface, pressure, exner, water_vapor, &
                  cloud_water_mass, cloud_ice_mass
    type(v2d_t) :: accumulated_precipitation
    type(v2_t) :: accumulated_convective_pcp
    type(tend_t) :: tend
    integer, pointer :: kpbl(:,:) => null()
  end type
  type cu_options_t
    real :: stochastic_cu, tendency_fraction, tend_qv_fraction, tend_qc_fraction, tend_th_fraction, tend_qi_fraction
  end type
  type physics_t
    integer :: convection
  end type
  type options_t
    type(cu_options_t) :: cu_options
    type(physics_t) :: physics
  end type
  type(domain_t), save :: dom
  type(options_t), save :: opt
  ! cu_driver.f90:24-35
  logical,allocatable, dimension(:,:) ::  CU_ACT_FLAG
  real,   allocatable, dimension(:,:) ::  XLAND, RAINCV, PRATEC
  real,   allocatable, dimension(:,:)::   CLDEFI
  real,   allocatable, dimension(:,:)::   CUBOT,CUTOP, CONVCLD
  real,   allocatable, dimension(:,:,:):: CCLDFRA, QCCONV, QICONV
  integer :: ids,ide,jds,jde,kds,kde
  integer :: ims,ime,jms,jme,kms,kme
  integer :: its,ite,jts,jte,kts,kte
  integer, allocatable, dimension(:,:) :: lowlyr
  logical :: bmj_rad_feedback
  real, allocatable, target, dimension(:,:,:) :: zeros_qc, zeros_qi, zeros_qs, zeros_qr, zeros_u, zeros_v
  integer, allocatable, target :: kpbl_store(:,:)
contains
  subroutine convect_body(domain, options, dt_in)
    type(domain_t),  intent(inout) :: domain
    type(options_t), intent(in)    :: options
    real, intent(in) :: dt_in
    integer :: j,itimestep,STEPCU
    real :: internal_dt
    itimestep = 1
    STEPCU = 1
@ZERO@
@BMJDRV@
    internal_dt = dt_in
@APPLY@
        enddo
  end subroutine

  subroutine ref_cu_init(nx, nz, ny, its_, ite_, jts_, jte_, land_mask) bind(C, name="ref_cu_init")
    integer(c_int), value :: nx, nz, ny, its_, ite_, jts_, jte_
    integer(c_int), dimension(nx,ny) :: land_mask
    real, allocatable, dimension(:,:,:) :: a, b, c, d
    ims = 1; ime = nx; kms = 1; kme = nz; jms = 1; jme = ny
    ids = 1; ide = nx + 1; kds = 1; kde = nz + 1; jds = 1; jde = ny + 1
    its = its_; ite = ite_; jts = jts_; jte = jte_; kts = 1; kte = nz
    if (allocated(XLAND)) deallocate(CU_ACT_FLAG, XLAND, RAINCV, PRATEC, CLDEFI, CUBOT, CUTOP, CONVCLD, CCLDFRA, QCCONV, QICONV, lowlyr, &
                                     zeros_qc, zeros_qi, zeros_qs, zeros_qr, zeros_u, zeros_v, kpbl_store)
    allocate(CU_ACT_FLAG(ims:ime,jms:jme), source=.False.)
    allocate(RAINCV(ims:ime,jms:jme)); allocate(PRATEC(ims:ime,jms:jme)); RAINCV = 0; PRATEC = 0
    allocate(XLAND(ims:ime,jms:jme))
    XLAND = land_mask                                   ! cu_driver.f90:139
    where(land_mask == 0) XLAND = 2                     ! :140
    allocate(CLDEFI(ims:ime,jms:jme)); allocate(CUBOT(ims:ime,jms:jme)); allocate(CUTOP(ims:ime,jms:jme)); allocate(CONVCLD(ims:ime,jms:jme))
    allocate(CCLDFRA(ims:ime,jms:jme,kms:kme)); allocate(QCCONV(ims:ime,jms:jme,kms:kme)); allocate(QICONV(ims:ime,jms:jme,kms:kme))
    allocate(lowlyr(ims:ime,jms:jme)); allocate(kpbl_store(ims:ime,jms:jme))
    lowlyr = 1; kpbl_store = 10                         ! :221-222
    dom%kpbl => kpbl_store
    CLDEFI = AVGEFI; CUBOT = 0; CUTOP = 0; CONVCLD = 0  ! (BMJINIT sets CLDEFI on the tile only; the rest is never read)
    bmj_rad_feedback = .true.                           ! :228
    allocate(a(ims:ime,kms:kme,jms:jme)); allocate(b(ims:ime,kms:kme,jms:jme)); allocate(c(ims:ime,kms:kme,jms:jme)); allocate(d(ims:ime,kms:kme,jms:jme))
    call BMJINIT(a, b, c, d, CLDEFI, lowlyr, cp, r_d, .false., .true., ids, ide, jds, jde, kds, kde, ims, ime, jms, jme, kms, kme, &
                 its, ite, jts, jte, kts, kte)          ! :230-243
    allocate(zeros_qc(ims:ime,kms:kme,jms:jme)); allocate(zeros_qi(ims:ime,kms:kme,jms:jme)); allocate(zeros_qs(ims:ime,kms:kme,jms:jme))
    allocate(zeros_qr(ims:ime,kms:kme,jms:jme)); allocate(zeros_u(ims:ime,kms:kme,jms:jme)); allocate(zeros_v(ims:ime,kms:kme,jms:jme))
    zeros_qc = 0; zeros_qi = 0; zeros_qs = 0; zeros_qr = 0; zeros_u = 0; zeros_v = 0
    dom%tend%qc => zeros_qc; dom%tend%qi => zeros_qi; dom%tend%qs => zeros_qs; dom%tend%qr => zeros_qr
    dom%tend%u => zeros_u; dom%tend%v => zeros_v
    opt%physics%convection = kCU_BMJ
    opt%cu_options%stochastic_cu = kNO_STOCHASTIC
  end subroutine

  subroutine ref_cu_tables(qs0_, sqs_, ptbl_, the0_, sthe_, ttbl_, the0q_, stheq_, ttblq_, avgefi_, efimn_) bind(C, name="ref_cu_tables")
    real(c_float) :: qs0_(JTB), sqs_(JTB), ptbl_(ITB,JTB), the0_(ITB), sthe_(ITB), ttbl_(JTB,ITB), the0q_(ITBQ), stheq_(ITBQ), ttblq_(JTBQ,ITBQ)
    real(c_float) :: avgefi_, efimn_
    qs0_ = QS0; sqs_ = SQS; ptbl_ = PTBL; the0_ = THE0; sthe_ = STHE; ttbl_ = TTBL; the0q_ = THE0Q; stheq_ = STHEQ; ttblq_ = TTBLQ
    avgefi_ = AVGEFI; efimn_ = EFIMN
  end subroutine

  subroutine ref_cu_convect(nx, nz, ny, dt, t, qv, th, qc, qi, pmid, pint, pii, rho, dz, cldefi_, raincv_, cutop_, cubot_, tend_th, tend_qv, &
                            acc, accc, tf, fqv, fqc, fth, fqi) bind(C, name="ref_cu_convect")
    integer(c_int), value :: nx, nz, ny
    real(c_float), value :: dt, tf, fqv, fqc, fth, fqi
    real(c_float), dimension(nx,nz,ny), target :: t, qv, th, qc, qi, pmid, pint, pii, rho, dz, tend_th, tend_qv
    real(c_float), dimension(nx,ny) :: cldefi_, raincv_, cutop_, cubot_
    real(c_double), dimension(nx,ny), target :: acc
    real(c_float), dimension(nx,ny), target :: accc
    dom%temperature%data_3d => t; dom%water_vapor%data_3d => qv; dom%potential_temperature%data_3d => th
    dom%cloud_water_mass%data_3d => qc; dom%cloud_ice_mass%data_3d => qi; dom%pressure%data_3d => pmid
    dom%pressure_interface%data_3d => pint; dom%exner%data_3d => pii; dom%density%data_3d => rho; dom%dz_interface%data_3d => dz
    dom%tend%th => tend_th; dom%tend%qv => tend_qv
    dom%accumulated_precipitation%data_2dd => acc; dom%accumulated_convective_pcp%data_2d => accc
    opt%cu_options%tendency_fraction = tf; opt%cu_options%tend_qv_fraction = fqv; opt%cu_options%tend_qc_fraction = fqc
    opt%cu_options%tend_th_fraction = fth; opt%cu_options%tend_qi_fraction = fqi
    CLDEFI = cldefi_; RAINCV = raincv_; CUTOP = cutop_; CUBOT = cubot_
    call convect_body(dom, opt, dt)
    cldefi_ = CLDEFI; raincv_ = RAINCV; cutop_ = CUTOP; cubot_ = CUBOT
  end subroutine
end module
"""


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
    cu = open(os.path.join(REF, "src", "physics", "cu_driver.f90")).readlines()
    conv = next(n for n, l in enumerate(cu) if l.lstrip().startswith("subroutine convect("))
    zero, z_end = excerpt(cu, "do j=jts,jte", "enddo", 272, "the zeroing loop", conv)
    assert "RAINCV(:,j)     = 0" in zero and "domain%tend%v(:,:,j)  = 0" in zero
    drv, _ = excerpt(cu, "CALL BMJDRV(", "                )", 434, "the call of BMJDRV", z_end)
    assert "rqvcuten=domain%tend%qv" in drv and "KTE=kte-1" in drv
    app, _ = excerpt(cu, "do j=jts,jte", "domain%accumulated_convective_pcp%data_2d(:,j) = domain%accumulated_convective_pcp%data_2d(:,j) + RAINCV(:,j)",
                     483, "the tendency loop", z_end + 1)
    return SHIM.replace("@ZERO@", zero).replace("@BMJDRV@", drv).replace("@APPLY@", app)


def unprivate_bmj(tmp):
    """a copy of cu_bmj.f90 whose table declarations have lost their PRIVATE attribute, in tmp"""
    orig = open(os.path.join(REF, "src", "physics", "cu_bmj.f90")).readlines()
    new = [l.replace(",PRIVATE,SAVE ::", ",SAVE ::") if ("REAL,DIMENSION(" in l and ",PRIVATE,SAVE ::" in l) else l for l in orig]
    changed = [n for n in range(len(orig)) if orig[n] != new[n]]
    names = "".join(orig[n].split("::")[1] for n in changed).replace("\n", ",").replace(" ", "")
    assert len(changed) == 6 and sorted(x for x in names.split(",") if x) == sorted(["STHE", "THE0", "QS0", "SQS", "STHEQ", "THE0Q", "PTBL", "TTBL", "TTBLQ"]), \
        f"cu_bmj.f90: the table declarations are not the six lines expected ({changed})"
    path = os.path.join(tmp, "cu_bmj.f90")
    open(path, "w").writelines(new)
    return path


def build_reference(tmp):
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-w"]
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    objs = []
    for f in (os.path.join(src, "constants", "icar_constants.f90"), os.path.join(src, "constants", "wrf_constants.f90"), unprivate_bmj(tmp)):
        o = os.path.basename(f)[:-4] + ".o"
        run([FC] + flags + [f, "-o", o]); objs.append(o)
    open(os.path.join(tmp, "cu_shim.f90"), "w").write(shim_text())
    run([FC] + flags + ["cu_shim.f90", "-o", "cu_shim.o"]); objs.append("cu_shim.o")
    run([FC, "-shared", "-o", "libcuref.so"] + objs)
    return ctypes.CDLL(os.path.join(tmp, "libcuref.so"))


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def ref_init(L, c, tile=None):
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or B.tile_of(c)
    ci = ctypes.c_int
    L.ref_cu_init(ci(nx), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), _p(c["land_mask"]))


def ref_tables(L):
    out = {name: np.zeros(shape, np.float32) for name, shape in B.TABLES}
    a, e = ctypes.c_float(), ctypes.c_float()
    L.ref_cu_tables(*[_p(out[name]) for name, _ in B.TABLES], ctypes.byref(a), ctypes.byref(e))
    return out, a.value, e.value


def ref_call(L, c, A, n):
    """call n of the carried sequence with the reference's code"""
    ny, nz, nx = c["density"].shape
    if n:
        B.rediagnose(c, A)
    ci, cf = ctypes.c_int, ctypes.c_float
    fq = c["fractions"]
    L.ref_cu_convect(ci(nx), ci(nz), ci(ny), cf(B.DT[n]), _p(A["temperature"]), _p(A["water_vapor"]), _p(A["potential_temperature"]),
                     _p(A["cloud_water"]), _p(A["cloud_ice"]), _p(c["pressure"]), _p(c["pressure_interface"]), _p(c["exner"]), _p(c["density"]),
                     _p(c["dz_interface"]), _p(A["cldefi"]), _p(A["raincv"]), _p(A["cutop"]), _p(A["cubot"]), _p(A["tend_th"]), _p(A["tend_qv"]),
                     _p(A["accumulated_precipitation"]), _p(A["accumulated_convective_pcp"]), cf(c["tendency_fraction"]), cf(fq[0]), cf(fq[1]),
                     cf(fq[2]), cf(fq[3]))


def differing(A, O):
    return {k: B.bitdiff(A[k], O[k]) for k in B.STATE3 + B.STATE2 + ["accumulated_precipitation"]}


def columns(c, A):
    """(deep, shallow, none) column counts of the tile after a call, from the reference's own results"""
    rain = B.owned(c, A["raincv"])
    tend = (B.owned(c, A["tend_th"]) != 0).any(axis=1) | (B.owned(c, A["tend_qv"]) != 0).any(axis=1)
    deep = rain > 0
    return int(deep.sum()), int((tend & ~deep).sum()), int((~tend & ~deep).sum()), int(rain.size)


def make(L, name, write=True):
    p = B.CASES[name]
    c = B.make_case(**p)
    ref_init(L, c)
    A, O = B.state(c), B.state(c)
    out = {"input_fingerprint": np.float64(B.fingerprint(c))}
    same, counts = True, []
    for n in range(B.CALLS):
        ref_call(L, c, A, n)
        B.run_oracle(c, O, n)
        d = differing(A, O)
        same = same and not any(d.values())
        counts.append(columns(c, A))
        for k in B.STATE3 + B.STATE2 + ["accumulated_precipitation"]:
            assert np.isfinite(A[k]).all(), f"{name}: the reference's {k} is not finite after call {n + 1}"
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(A[k]))
        for k in B.STATE2 + ["accumulated_precipitation", "tend_th", "tend_qv"]:
            out[f"call{n + 1}_{k}"] = A[k].copy()
        if any(d.values()): print("   call", n + 1, "differing bits:", {k: v for k, v in d.items() if v})
    for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice"):
        out[f"call{B.CALLS}_{k}"] = A[k].copy()
    ce = B.owned(c, A["cldefi"])
    print(name, "restatement == reference:", same, "(deep, shallow, none, columns) per call:", counts,
          "CLDEFI", float(ce.min()), float(ce.max()))
    if write and same:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), counts=np.array(counts), **out)
    return same


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_bmj: the reference sources are not present")
    write = "--dry" not in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(B.CASES)
    with tempfile.TemporaryDirectory(prefix="icar_curef_") as tmp:
        L = build_reference(tmp)
        c0 = B.make_case(**B.CASES[names[0]])
        ref_init(L, c0)
        T, avgefi, efimn = ref_tables(L)
        mine = B.tables()
        td = {k: B.bitdiff(T[k], mine[k]) for k in T}
        print("tables: differing bits", td, "AVGEFI", avgefi, "EFIMN", efimn)
        ok = not any(td.values()) and np.float32(avgefi) == np.float32(B.AVGEFI()) and np.float32(efimn) == np.float32(B.EFIMN())
        if write and ok:
            np.savez_compressed(os.path.join(HERE, "cu_bmj_tables.npz"), avgefi=np.float32(avgefi), efimn=np.float32(efimn), **T)
        res = [make(L, n, write) for n in names]
        sys.exit(0 if ok and all(res) else 1)

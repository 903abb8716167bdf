#!/usr/bin/env python
"""Golden vectors of the surface-flux slot under tests/golden/sfc_basic_*.npz made by RUNNING THE REFERENCE'S OWN STATEMENTS, compiled
with the flags and interface modules of oracle/build_ref.sh up to options_h, in a temporary directory outside the repository.

How each range is pinned:
  water_simple            src/physics/water_simple.f90 WHOLE, from a temporary copy in which two tokens are repaired (this compiler
                          refuses the file as it stands): the stray comma that ends `use data_structures,` and the `module` of
                          `module subroutine water_simple` inside a plain module.  The generator asserts that exactly those two
                          lines differ from the original.
  apply_fluxes            src/physics/lsm_driver.f90, the subroutine from `subroutine apply_fluxes(domain,dt)` to its `end
                          subroutine`, the nz search included, EXCERPTED at generation time into a shim module of the
                          generator's own; lsm_driver.f90 as a whole uses Noah, Noah-MP, the lake model and a live domain_t with
                          coarray members, which nothing here can build or run.
  windspd, where(wind==0) the two statements of lsm / calc_exchange_coefficient, excerpted the same way; z_atm of lsm_init likewise.
  the 10 m diagnostics    src/main/time_step.f90, from `if (associated(domain%roughness_z0%data_2d)) then` to the `endif` behind the
                          master ustar, excerpted the same way.
The ranges are found by their text; the line numbers quoted in the sources are only checked to lie within 40 lines.  The shim's
domain_t holds `real, pointer` arrays under the reference's member names (data_3d / data_2d; ustar allocatable), as variable_t does.
The gate (REAL(8) clock arithmetic, lsm_driver.f90:1016-1023) is four lines of control flow and is restated, not excerpted.

Every case of tests/sfc_oracle.py:CASES runs CALLS carried calls.  Stored: SHA-256 of every carried field after every call, the 2-D
fields in full, the lowest levels of the two 3-D fields, and the shares of the branches as the CPU restatement flags them.  The
generator also runs the restatement with each way of forming sum(dz(i,kts:k-1,j)) and asserts that exactly tests/sfc_oracle.py's
SUM_MODE reproduces the compiled reference on every case, and that every reference output is finite.  Only runs where the reference
is present; tests/test_sfc_oracle.py pins the restatement to these files everywhere."""
import ctypes
import hashlib
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
import sfc_oracle as S  # noqa: E402

REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402
MODULES = ["constants/icar_constants", "constants/wrf_constants", "utilities/time_delta_obj", "utilities/time_h", "main/data_structures",
           "objects/opt_types", "objects/options_h"]
LOWEST = 4                       # levels of the 3-D fields stored in full

SHIM = """
module sfc_shim
  use iso_c_binding
  use icar_constants
  use options_interface, only: options_t
  use module_water_simple, only: water_simple
  implicit none
  type v3_t
    real, pointer :: data_3d(:,:,:) => null()
  end type
  type v2_t
    real, pointer :: data_2d(:,:) => null()
  end type
  type domain_t
    type(v3_t) :: dz_interface, density, exner, potential_temperature, water_vapor, z, u_mass, v_mass
    type(v2_t) :: sensible_heat, latent_heat, u_10m, v_10m, roughness_z0, terrain
    real, allocatable :: ustar(:,:)
  end type
  type(options_t), save :: options
  type(domain_t), save :: dom
@SMALL_QV@
  real, allocatable, dimension(:,:) :: dTemp, lhdQV, windspd, lastw, currw, z_atm
  real :: lh_feedback_fraction, sh_feedback_fraction, sfc_layer_thickness
  integer :: ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte
contains
@APPLY_FLUXES@
  subroutine zero_wind(wind)
    real, dimension(:,:), intent(inout) :: wind
@WHERE_WIND@
  end subroutine
  subroutine gated(domain)
    type(domain_t), intent(inout) :: domain
@WINDSPD@
    call zero_wind(windspd)
  end subroutine
  subroutine first_level_height(domain)
    type(domain_t), intent(inout) :: domain
@Z_ATM@
  end subroutine
  subroutine diag(domain)
    type(domain_t), intent(inout) :: domain
    associate(u_mass => domain%u_mass%data_3d, v_mass => domain%v_mass%data_3d)
@DIAG@
    end associate
  end subroutine

  subroutine bounds(nx, nz, ny)
    integer, intent(in) :: nx, nz, ny
    ims = 1; ime = nx; kms = 1; kme = nz; jms = 1; jme = ny
  end subroutine

  subroutine ref_sfc_diag(nx, nz, ny, z, terrain, z0, u_mass, v_mass, u10, v10, ustar) bind(C, name="ref_sfc_diag")
    integer(c_int), value :: nx, nz, ny
    real(c_float), dimension(nx,nz,ny), target :: z, u_mass, v_mass
    real(c_float), dimension(nx,ny), target :: terrain, z0, u10, v10
    real(c_float), dimension(nx,ny) :: ustar
    call bounds(nx, nz, ny)
    dom%z%data_3d => z; dom%u_mass%data_3d => u_mass; dom%v_mass%data_3d => v_mass
    dom%terrain%data_2d => terrain; dom%roughness_z0%data_2d => z0; dom%u_10m%data_2d => u10; dom%v_10m%data_2d => v10
    if (allocated(dom%ustar)) deallocate(dom%ustar)
    allocate(dom%ustar(nx,ny)); dom%ustar = ustar
    if (allocated(lastw)) deallocate(lastw, currw)
    allocate(lastw(ims+1:ime-1, jms+1:jme-1)); allocate(currw(ims+1:ime-1, jms+1:jme-1))
    call diag(dom)
    ustar = dom%ustar
  end subroutine

  subroutine ref_sfc_gated(nx, nz, ny, u10, v10, sst, psfc, ustar, qv, temperature, z, terrain, landmask, sensible, latent, z0, &
                           qsfc, qfx, tskin, run_water) bind(C, name="ref_sfc_gated")
    integer(c_int), value :: nx, nz, ny, run_water
    real(c_float), dimension(nx,nz,ny), target :: qv, temperature, z
    real(c_float), dimension(nx,ny), target :: u10, v10, terrain
    real(c_float), dimension(nx,ny) :: sst, psfc, ustar, sensible, latent, z0, qsfc, qfx, tskin
    integer(c_int), dimension(nx,ny) :: landmask
    call bounds(nx, nz, ny)
    kts = 1
    dom%z%data_3d => z; dom%terrain%data_2d => terrain; dom%u_10m%data_2d => u10; dom%v_10m%data_2d => v10
    if (allocated(windspd)) deallocate(windspd, z_atm)
    allocate(windspd(ims:ime,jms:jme)); allocate(z_atm(ims:ime,jms:jme))
    windspd = 3
    call gated(dom)
    if (run_water /= 0) then
      call first_level_height(dom)
      options%physics%watersurface = kWATER_SIMPLE
      call water_simple(options, sst, psfc, windspd, ustar, qv, temperature, sensible, latent, z_atm, z0, landmask, qsfc, qfx, tskin, landmask)
    endif
  end subroutine

  subroutine ref_sfc_apply(nx, nz, ny, th, qv, density, pii, dz, sensible, latent, dt, sh, lh, thick, its_, ite_, jts_, jte_, kts_, kte_) &
                           bind(C, name="ref_sfc_apply")
    integer(c_int), value :: nx, nz, ny, its_, ite_, jts_, jte_, kts_, kte_
    real(c_float), value :: dt, sh, lh, thick
    real(c_float), dimension(nx,nz,ny), target :: th, qv, density, pii, dz
    real(c_float), dimension(nx,ny), target :: sensible, latent
    call bounds(nx, nz, ny)
    its = its_; ite = ite_; jts = jts_; jte = jte_; kts = kts_; kte = kte_
    sh_feedback_fraction = sh; lh_feedback_fraction = lh; sfc_layer_thickness = thick
    dom%potential_temperature%data_3d => th; dom%water_vapor%data_3d => qv; dom%density%data_3d => density
    dom%exner%data_3d => pii; dom%dz_interface%data_3d => dz
    dom%sensible_heat%data_2d => sensible; dom%latent_heat%data_2d => latent
    if (allocated(dTemp)) deallocate(dTemp, lhdQV)
    allocate(dTemp(its:ite,jts:jte)); allocate(lhdQV(its:ite,jts:jte))
    dTemp = 0; lhdQV = 0
    call apply_fluxes(dom, dt)
  end subroutine
end module
"""


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def excerpt(lines, first, last, near, what):
    """the lines from the first one containing `first` to the first one at or behind it containing `last`, inclusive"""
    a = next((n for n, l in enumerate(lines) if first in l), None)
    assert a is not None, f"{what}: `{first}` not found in the reference"
    b = next((n for n in range(a, len(lines)) if last in lines[n]), None)
    assert b is not None, f"{what}: `{last}` not found behind it"
    assert abs(a + 1 - near) <= 40, f"{what}: found at line {a + 1}, expected near {near}"
    return "".join(lines[a:b + 1])


def shim_text():
    src = os.path.join(REF, "src")
    lsm = open(os.path.join(src, "physics", "lsm_driver.f90")).readlines()
    ts = open(os.path.join(src, "main", "time_step.f90")).readlines()
    parts = {
        "SMALL_QV": excerpt(lsm, "real, parameter :: SMALL_QV", "SMALL_QV", 87, "SMALL_QV"),
        "APPLY_FLUXES": excerpt(lsm, "subroutine apply_fluxes(domain,dt)", "end subroutine apply_fluxes", 361, "apply_fluxes"),
        "WHERE_WIND": excerpt(lsm, "where(wind==0) wind=1e-5", "where(wind==0)", 251, "where(wind==0)"),
        "WINDSPD": excerpt(lsm, "windspd = sqrt(domain%u_10m%data_2d**2 + domain%v_10m%data_2d**2)", "windspd", 1028, "windspd"),
        "Z_ATM": excerpt(lsm, "z_atm = domain%z%data_3d(:,kts,:) - domain%terrain%data_2d", "z_atm", 992, "z_atm"),
        "DIAG": excerpt(ts, "if (associated(domain%roughness_z0%data_2d)) then", "sqrt(u_mass(ims+1:ime-1,kms,jms+1:jme-1)**2", 144, "10 m diagnostics"),
    }
    parts["DIAG"] += "        endif\n"            # the `endif` of `if (allocated(domain%ustar))`, the line behind the excerpt's last
    d = next(n for n, l in enumerate(ts) if "sqrt(u_mass(ims+1:ime-1,kms,jms+1:jme-1)**2" in l)
    assert ts[d + 1].strip() == "endif", "10 m diagnostics: the master ustar is no longer the last statement of its block"
    text = SHIM
    for k, v in parts.items():
        text = text.replace("@" + k + "@", v)
    return text


def repaired_water_simple(tmp):
    """a copy of water_simple.f90 with its two syntax slips repaired, in tmp"""
    orig = open(os.path.join(REF, "src", "physics", "water_simple.f90")).readlines()
    new = list(orig)
    a = next(n for n, l in enumerate(orig) if l.strip() == "use data_structures,")
    b = next(n for n, l in enumerate(orig) if l.lstrip().startswith("module subroutine water_simple("))
    new[a] = orig[a].replace("use data_structures,", "use data_structures")
    new[b] = orig[b].replace("module subroutine", "subroutine", 1)
    assert [n for n in range(len(orig)) if orig[n] != new[n]] == sorted([a, b]) and len(new) == len(orig)
    path = os.path.join(tmp, "water_simple.f90")
    open(path, "w").writelines(new)
    return path


def build_reference(tmp):
    """libsfcref.so in tmp; returns its path (load() gives every case a copy: apply_fluxes keeps nz in a SAVE variable)"""
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-fcoarray", "-w", "-DUSE_ASSERTIONS=.false.", "-I" + os.path.join(src, "physics"), "-I" + os.path.join(src, "utilities")]
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    run([FC, "-c", "-O2", "-fPIC", "-w", os.path.join(ROOT, "oracle", "ref_link_stubs.f90"), "-o", "ref_link_stubs.o"])
    run(["gcc", "-c", "-fPIC", os.path.join(ROOT, "oracle", "ref_link_stubs.c"), "-o", "ref_link_stubs_c.o"])
    objs = ["ref_link_stubs.o", "ref_link_stubs_c.o"]
    for m in MODULES:
        o = os.path.basename(m) + ".o"
        run([FC] + flags + [os.path.join(src, m + ".f90"), "-o", o])
        objs.append(o)
    run([FC] + flags + [repaired_water_simple(tmp), "-o", "water_simple.o"])
    objs.append("water_simple.o")
    open(os.path.join(tmp, "sfc_shim.f90"), "w").write(shim_text())
    run([FC] + flags + ["sfc_shim.f90", "-o", "sfc_shim.o"])
    objs.append("sfc_shim.o")
    und = subprocess.check_output(["nm", "-u"] + objs, cwd=tmp, text=True)
    dfn = subprocess.check_output(["nm", "--defined-only"] + objs, cwd=tmp, text=True)
    undef = {l.split()[1] for l in und.splitlines() if len(l.split()) == 2 and l.split()[0] == "U" and l.split()[1].startswith("_QM")}
    defined = {l.split()[2] for l in dfn.splitlines() if len(l.split()) == 3}
    open(os.path.join(tmp, "defsyms.rsp"), "w").write("\n".join(f"-Wl,--defsym,{s}=0" for s in sorted(undef - defined)))
    run([FC, "-shared", "-o", "libsfcref.so"] + objs + ["@defsyms.rsp"])
    return os.path.join(tmp, "libsfcref.so")


_copies = [0]


def load(path):
    """a private copy of the library: a fresh `nz` for apply_fluxes' SAVE variable"""
    _copies[0] += 1
    mine = path[:-3] + f"_{_copies[0]}.so"
    shutil.copy(path, mine)
    return ctypes.CDLL(mine)


def run_reference(L, c, A, n=0, tile=None):
    """call n of the carried sequence with the reference's statements; the gate is S.gate's"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ci, cf = ctypes.c_int, ctypes.c_float
    dims = (ci(nx), ci(nz), ci(ny))
    L.ref_sfc_diag(*dims, p(c["z"]), p(c["terrain"]), p(A["roughness_z0"]), p(c["u_mass"]), p(c["v_mass"]), p(A["u_10m"]), p(A["v_10m"]), p(A["ustar"]))
    if S.gate(c, A, S.CLOCK[n]):
        L.ref_sfc_gated(*dims, p(A["u_10m"]), p(A["v_10m"]), p(c["sst"]), p(c["surface_pressure"]), p(A["ustar"]), p(A["water_vapor"]),
                        p(c["temperature"]), p(c["z"]), p(c["terrain"]), p(c["land_mask"]), p(A["sensible_heat"]), p(A["latent_heat"]),
                        p(A["roughness_z0"]), p(A["qsfc"]), p(A["qfx"]), p(A["skin_temperature"]), ci(int(c["watersurface"] == S.kWATER_SIMPLE)))
    L.ref_sfc_apply(*dims, p(A["potential_temperature"]), p(A["water_vapor"]), p(c["density"]), p(c["exner"]), p(c["dz_interface"]),
                    p(A["sensible_heat"]), p(A["latent_heat"]), cf(c["sfc_dt"] * (n + 1)), cf(c["sh_feedback_fraction"]), cf(c["lh_feedback_fraction"]),
                    cf(c["sfc_layer_thickness"]), ci(its), ci(ite), ci(jts), ci(jte), ci(c["kts"]), ci(nz))


def differing(A, B):
    return {k: S.bitdiff(A[k], B[k]) for k in S.STATE3 + S.STATE2}


def shares(c, wf, af):   # (tests/test_sfc_oracle.py recomputes them with this function)
    """the branch shares of a case: water_simple's over its relevant cells in the first call, apply_fluxes' over the layer's cells"""
    W, F = S.WFLAGS, S.AFLAGS
    cell = (wf & W["cell"]) != 0
    water = cell & ((wf & W["water"]) != 0)
    out = {"water": float(((wf & W["water"]) != 0)[cell].mean()) if cell.any() else 0.0, "wind0": float(((wf & W["wind0"]) != 0).mean())}
    for k in ("ice", "clip", "ri_neg", "ustar_floor"):
        out[k] = float(((wf & W[k]) != 0)[water].mean()) if water.any() else 0.0
    upper = (af & F["upper"]) != 0
    layer = (af & F["layer"]) != 0
    out["min1"] = float(((af & F["min1"]) != 0)[upper].mean()) if upper.any() else 0.0
    out["max0"] = float(((af & F["max0"]) != 0)[upper].mean()) if upper.any() else 0.0
    out["floor_layer"] = float(((af & F["floor"]) != 0)[layer].mean())
    above = np.zeros_like(layer); above[:, c["kts"] + S.layers(c, c["kts"]) + 2:, :] = True      # at least two levels above the loop's last
    out["floor_above"] = float(((af & F["floor"]) != 0)[above].mean()) if above.any() else 0.0
    return out


def make(path, name, write=True):
    p = S.CASES[name]
    c = S.make_case(**p)
    A = S.state(c)
    B = {m: S.state(c) for m in (0, 1, 2)}
    out = {"input_fingerprint": np.float64(S.fingerprint(c)), "layers": np.int32(S.layers(c, c["kts"]))}
    L = load(path)
    same = {m: True for m in B}
    sh, gates = None, []
    for n in range(S.CALLS):
        run_reference(L, c, A, n)
        for m in B:
            is_open, wf, af = S.run_oracle(c, B[m], n, flags=True, sum_mode=m)
            same[m] = same[m] and not any(differing(A, B[m]).values())
            if m == S.SUM_MODE and n == 0: sh = shares(c, wf, af)
        gates.append(bool(is_open))
        for k in S.STATE3 + S.STATE2:
            assert np.isfinite(A[k]).all(), f"{name}: the reference's {k} is not finite after call {n + 1}"
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(A[k]))
        for k in S.STATE2:
            out[f"call{n + 1}_{k}"] = A[k].copy()
        for k in S.STATE3:
            out[f"call{n + 1}_{k}_lowest"] = A[k][:, :LOWEST, :].copy()
    ok = same[S.SUM_MODE]
    print(name, "restatement == reference per sum mode:", same, "gates", gates, {k: round(v, 3) for k, v in sh.items()}, "layers", int(out["layers"]))
    if write and ok:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), shares=np.array(json.dumps(sh)),
                            gates=np.array(gates), **out)
    return ok, same


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_sfc: the reference sources are not present")
    with tempfile.TemporaryDirectory(prefix="icar_sfcref_") as tmp:
        path = build_reference(tmp)
        res = [make(path, n) for n in (sys.argv[1:] or S.CASES)]
        # the sum's form is settled only if some case tells the candidates apart
        for m in (0, 1, 2):
            if m != S.SUM_MODE:
                assert not all(s[m] for _, s in res), f"no case tells sum mode {m} from mode {S.SUM_MODE}: the fixtures do not settle it"
        sys.exit(0 if all(ok for ok, _ in res) else 1)

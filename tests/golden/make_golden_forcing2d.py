#!/usr/bin/env python
"""Golden vectors of the 2-D forced variables under tests/golden/forcing2d_*.npz made by RUNNING THE REFERENCE'S OWN STATEMENTS, compiled
with the flags and interface modules tests/golden/make_golden_forcing.py uses, in a temporary directory outside the repository.

How each range is pinned:
  geo_LUT, geo_interp2d   src/utilities/geo_reader.f90 WHOLE and unmodified (module geo)
  the 2-D delta           src/objects/domain_obj.f90 `var_to_update%dqdt_2d = (var_to_update%dqdt_2d - var_to_update%data_2d) / dt%seconds()`
  the 2-D apply           `var_to_update%data_2d = var_to_update%data_2d + (var_to_update%dqdt_2d * dt%seconds())`
  the precipitation sum   `this%accumulated_precipitation%data_2dd = this%accumulated_precipitation%data_2dd + (this%external_precipitation%data_2d * dt%seconds())`
each statement EXCERPTED at generation time by its text into a shim module of the generator's own (domain_obj.f90 as a whole is a
submodule that needs NetCDF and coarrays), with the reference's own time_delta_t (src/utilities/time_delta_obj.f90).  The line numbers
quoted here are only checked to lie within 60 lines.

The geometry is that of the six cases of tests/forcing_oracle.py:CASES (and, not stored, of its two EXTRA_SEEDS); the generator's own
geo_LUT must reproduce the geolut the forcing_*.npz fixtures store, bit for bit, and the 2-D fixtures keep only a checksum of it.  Every
case runs tests/forcing2d_oracle.py:run_oracle's chain: an initial interpolation, two forcing intervals of interpolate (update) and delta,
three and two applies with different dt.  The restatement is run with plain product-sums and with FMAs, and nothing is written unless
the plain form differs from the compiled reference in 0 bits of every array after every stage of all eight cases and the FMA form
differs somewhere.  Every cell of every array is compared.  Stored per fixture: every stage of the reference in full.
Only runs where the reference is present; tests/test_forcing2d_oracle.py pins the restatement to these files everywhere."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import forcing_oracle as FO  # noqa: E402
import forcing2d_oracle as F2  # noqa: E402
import make_golden_forcing as MG  # noqa: E402   (excerpt(), the compiler and the reference's location)

REF, FC = MG.REF, MG.FC
MODULES = ["constants/icar_constants", "constants/wrf_constants", "utilities/time_delta_obj", "utilities/time_h", "main/data_structures",
           "utilities/geo_reader"]

SHIM = """
module forcing2d_shim
  use iso_c_binding
  use data_structures
  use time_delta_object, only : time_delta_t
  use geo, only : geo_LUT, geo_interp2d
  implicit none
  type variable_t
    real, pointer :: data_2d(:,:) => null()
    real, pointer :: dqdt_2d(:,:) => null()
    real(kind=8), pointer :: data_2dd(:,:) => null()
  end type
  type domain_t
    type(variable_t) :: accumulated_precipitation, external_precipitation
  end type
  type(interpolable_type), save :: lo
contains
  subroutine delta(var_to_update, dt)
    type(variable_t), intent(inout) :: var_to_update
    type(time_delta_t), intent(in) :: dt
@DELTA@
  end subroutine

  subroutine apply(var_to_update, dt)
    type(variable_t), intent(inout) :: var_to_update
    type(time_delta_t), intent(in) :: dt
@APPLY@
  end subroutine

  subroutine precip(this, dt)
    type(domain_t), intent(inout) :: this
    type(time_delta_t), intent(in) :: dt
@PRECIP@
  end subroutine

  subroutine ref2_setup(nx, ny, nxf, nyf, hlat, hlon, llat, llon, gx, gy, gw) bind(C, name="ref2_setup")
    integer(c_int), value :: nx, ny, nxf, nyf
    real(c_float) :: hlat(nx,ny), hlon(nx,ny), llat(nxf,nyf), llon(nxf,nyf), gw(4,nx,ny)
    integer(c_int) :: gx(4,nx,ny), gy(4,nx,ny)
    type(interpolable_type) :: hi
    if (allocated(lo%lat)) deallocate(lo%lat, lo%lon, lo%geolut%x, lo%geolut%y, lo%geolut%w)
    allocate(hi%lat(nx,ny), hi%lon(nx,ny))
    hi%lat = hlat; hi%lon = hlon
    allocate(lo%lat(nxf,nyf), lo%lon(nxf,nyf))
    lo%lat = llat; lo%lon = llon
    call geo_LUT(hi, lo)
    gx = lo%geolut%x; gy = lo%geolut%y; gw = lo%geolut%w
  end subroutine

  subroutine ref2_interp(fieldout, nx, ny, fieldin, nxf, nyf) bind(C, name="ref2_interp")
    integer(c_int), value :: nx, ny, nxf, nyf
    real(c_float) :: fieldout(nx,ny), fieldin(nxf,nyf)
    call geo_interp2d(fieldout, fieldin, lo%geolut)
  end subroutine

  subroutine ref2_delta(dqdt, data, nx, ny, seconds) bind(C, name="ref2_delta")
    integer(c_int), value :: nx, ny
    real(c_double), value :: seconds
    real(c_float), target :: dqdt(nx,ny), data(nx,ny)
    type(variable_t) :: v
    type(time_delta_t) :: dt
    call dt%set(seconds=seconds)
    v%dqdt_2d => dqdt; v%data_2d => data
    call delta(v, dt)
  end subroutine

  subroutine ref2_apply(data, dqdt, nx, ny, seconds) bind(C, name="ref2_apply")
    integer(c_int), value :: nx, ny
    real(c_double), value :: seconds
    real(c_float), target :: dqdt(nx,ny), data(nx,ny)
    type(variable_t) :: v
    type(time_delta_t) :: dt
    call dt%set(seconds=seconds)
    v%dqdt_2d => dqdt; v%data_2d => data
    call apply(v, dt)
  end subroutine

  subroutine ref2_precip(acc, ext, nx, ny, seconds) bind(C, name="ref2_precip")
    integer(c_int), value :: nx, ny
    real(c_double), value :: seconds
    real(c_double), target :: acc(nx,ny)
    real(c_float), target :: ext(nx,ny)
    type(domain_t) :: d
    type(time_delta_t) :: dt
    call dt%set(seconds=seconds)
    d%accumulated_precipitation%data_2dd => acc; d%external_precipitation%data_2d => ext
    call precip(d, dt)
  end subroutine
end module
"""


def shim_text():
    dom = open(os.path.join(REF, "src", "objects", "domain_obj.f90")).readlines()
    one = lambda text, near, what: MG.excerpt(dom, text, "dt%seconds()", near, what)
    parts = {
        "DELTA": one("var_to_update%dqdt_2d = (var_to_update%dqdt_2d - var_to_update%data_2d) / dt%seconds()", 2356, "the 2-D delta"),
        "APPLY": one("var_to_update%data_2d = var_to_update%data_2d + (var_to_update%dqdt_2d * dt%seconds())", 2402, "the 2-D apply"),
        "PRECIP": one("this%accumulated_precipitation%data_2dd = this%accumulated_precipitation%data_2dd + (this%external_precipitation%data_2d * dt%seconds())",
                      2443, "the precipitation sum"),
    }
    text = SHIM
    for k, v in parts.items():
        assert v.count("\n") == 1, f"{k}: one statement expected, got\n{v}"
        text = text.replace("@" + k + "@", v)
    return text


def build_reference(tmp):
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-fcoarray", "-w", "-DUSE_ASSERTIONS=.false.", "-I" + os.path.join(src, "physics"), "-I" + os.path.join(src, "utilities")]

    def run(cmd):
        r = subprocess.run(cmd, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit("make_golden_forcing2d: " + " ".join(cmd[:3]) + " ... failed:\n" + r.stderr[-3000:])
    run([FC, "-c", "-O2", "-fPIC", "-w", os.path.join(ROOT, "oracle", "ref_link_stubs.f90"), "-o", "ref_link_stubs.o"])
    run(["gcc", "-c", "-fPIC", os.path.join(ROOT, "oracle", "ref_link_stubs.c"), "-o", "ref_link_stubs_c.o"])
    objs = ["ref_link_stubs.o", "ref_link_stubs_c.o"]
    for m in MODULES:
        o = os.path.basename(m) + ".o"
        run([FC] + flags + [os.path.join(src, m + ".f90"), "-o", o])
        objs.append(o)
    open(os.path.join(tmp, "forcing2d_shim.f90"), "w").write(shim_text())
    run([FC] + flags + ["forcing2d_shim.f90", "-o", "forcing2d_shim.o"])
    objs.append("forcing2d_shim.o")
    und = subprocess.check_output(["nm", "-u"] + objs, cwd=tmp, text=True)
    dfn = subprocess.check_output(["nm", "--defined-only"] + objs, cwd=tmp, text=True)
    undef = {l.split()[1] for l in und.splitlines() if len(l.split()) == 2 and l.split()[0] == "U" and l.split()[1].startswith("_QM")}
    defined = {l.split()[2] for l in dfn.splitlines() if len(l.split()) == 3}
    open(os.path.join(tmp, "defsyms.rsp"), "w").write("\n".join(f"-Wl,--defsym,{s}=0" for s in sorted(undef - defined)))
    run([FC, "-shared", "-o", "libforcing2dref.so"] + objs + ["@defsyms.rsp"])
    return ctypes.CDLL(os.path.join(tmp, "libforcing2dref.so"))


p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
ci, cd = ctypes.c_int, ctypes.c_double


def reference_lut(R, c3):
    """geo_LUT of the compiled reference for the mass grid of a 3-D case's geometry"""
    h = c3["hi"]
    ny, nx = h["lat"].shape
    nyf, nxf = c3["lo_lat"].shape
    G = {"x": np.empty((ny, nx, 4), np.int32), "y": np.empty((ny, nx, 4), np.int32), "w": np.empty((ny, nx, 4), np.float32)}
    R.ref2_setup(ci(nx), ci(ny), ci(nxf), ci(nyf), p(h["lat"]), p(h["lon"]), p(c3["lo_lat"]), p(c3["lo_lon"]), p(G["x"]), p(G["y"]), p(G["w"]))
    return G


def run_reference(R, c):
    """what F2.run_oracle computes (everything enabled), with the reference's statements; ref2_setup has been called for this case"""
    ny, nx = c["ny"], c["nx"]

    def interp(lo):
        out = np.full((ny, nx), np.nan, np.float32)
        R.ref2_interp(p(out), ci(nx), ci(ny), p(lo), ci(lo.shape[1]), ci(lo.shape[0]))
        return out
    out, data, dq = {}, {}, {}
    for v in F2.VARS:
        data[v] = interp(c["lo"][0][v])
        out[f"init_{v}"] = data[v].copy()
    acc = c["acc0"].copy()
    for n in (1, 2):
        for v in F2.VARS:
            dq[v] = interp(c["lo"][n][v])
            out[f"i{n}_pre_{v}"] = dq[v].copy()
        for v in F2.VARS:
            R.ref2_delta(p(dq[v]), p(data[v]), ci(nx), ci(ny), cd(F2.INTERVAL_DT[n - 1]))
            out[f"i{n}_dq_{v}"] = dq[v].copy()
        for k, dt in enumerate(F2.APPLY_DT[n - 1]):
            for v in F2.VARS:
                R.ref2_apply(p(data[v]), p(dq[v]), ci(nx), ci(ny), cd(dt))
            R.ref2_precip(p(acc), p(data["external_precipitation"]), ci(nx), ci(ny), cd(dt))
            for v in F2.VARS:
                out[f"i{n}_a{k}_{v}"] = data[v].copy()
            out[f"i{n}_a{k}_acc"] = acc.copy()
    return out


def make(R, L0, L1, name, params, stored, write):
    c3 = FO.make_inputs(**params)
    G = reference_lut(R, c3)
    if stored:                                                    # the geolut the forcing_*.npz fixture holds is this one
        f3, _ = FO.load_case(name)
        for k in ("x", "y", "w"):
            assert np.ascontiguousarray(G[k]).tobytes() == np.ascontiguousarray(f3["geo"][k]).tobytes(), f"{name}: geo_LUT does not reproduce the stored geolut%{k}"
    c = F2.make_inputs(name, params)
    c["G"] = G
    ref = run_reference(R, c)
    plain, fma = F2.run_oracle(c, L=L0), F2.run_oracle(c, L=L1)
    assert set(ref) == set(plain) == set(fma)
    for k, v in ref.items():
        assert np.isfinite(v).all(), f"{name}: the reference's {k} is not finite"
    d0 = {k: F2.bitdiff(ref[k], plain[k]) for k in ref}
    d1 = {k: F2.bitdiff(ref[k], fma[k]) for k in ref}
    ok = not any(d0.values())
    print(name, "plain differs in", sum(d0.values()), "elements, FMA in", sum(d1.values()), "of", sum(v.size for v in ref.values()),
          "| FMA stages that differ:", sum(1 for v in d1.values() if v), "of", len(d1))
    if not ok:
        print("   ", {k: v for k, v in d0.items() if v})
    if write and ok:
        out = {"lut_sha": np.array(F2.lut_sha(G)), "input_fingerprint": np.float64(F2.fingerprint(c))}
        out.update(ref)
        np.savez_compressed(os.path.join(HERE, F2.CASES[name] + ".npz"), **out)
    return ok, sum(d1.values())


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_forcing2d: the reference sources are not present")
    with tempfile.TemporaryDirectory(prefix="icar_forcing2dref_") as tmp:
        R = build_reference(tmp)
        L0 = ctypes.CDLL(F2.build(force=True, contract=False, out=os.path.join(tmp, "libf2_plain.so")))
        L1 = ctypes.CDLL(F2.build(force=True, contract=True, out=os.path.join(tmp, "libf2_fma.so")))
        assert L0.f2o_contract() == 0 and L1.f2o_contract() == 1
        cases = {**FO.CASES, **FO.EXTRA_SEEDS}
        dry = "--dry" in sys.argv
        # nothing is written unless all eight agree: a first pass without writing, then the six fixtures
        res = {n: make(R, L0, L1, n, q, n in FO.CASES, write=False) for n, q in cases.items()}
        good = all(ok for ok, _ in res.values())
        assert any(f for _, f in res.values()), "the FMA form reproduces the reference everywhere too: these inputs do not settle the form -- choose others"
        if good and not dry:
            for n, q in FO.CASES.items():
                make(R, L0, L1, n, q, True, write=True)
        sys.exit(0 if good else 1)

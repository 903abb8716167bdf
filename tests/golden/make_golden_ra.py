#!/usr/bin/env python
"""Golden vectors of the simple radiation scheme under tests/golden/ra_simple_*.npz made by RUNNING THE REFERENCE'S OWN MODULE:
src/physics/ra_simple.f90 compiled unmodified (the flags and interface modules of oracle/build_ref.sh up to domain_h, then
physics/mp_thompson, utilities/atm_utilities -- relative_humidity -- and physics/ra_simple) together with the bind(C) shim below, in
a temporary directory outside the repository; ra_simple runs CALLS times on each case of tests/ra_oracle.py:CASES with theta and
the three 2-D results carried from call to call, dt growing and the clock advancing.

The date.  ra_simple asks a Time_type for day_of_year(lon) and year_fraction(lon).  Their bodies live in time_obj.f90, which this
compiler does not build (REAL(16) formatted output); the generator supplies a submodule of its own that defines just these two
procedures with the arithmetic of time_obj.f90:404-480 (REAL(16) sums, the lon > 180 branch, the three calendars, mod(., 1.0)) on
`current_date_time` = days since 1 January 00:00 and the year's length, which the shim puts into `year_zero`.  The calendar
arithmetic that produces those two numbers (date -> modified Julian day) is not run: that part is unpinned.

Inputs are regenerated from the recorded recipe (a fingerprint detects drift).  Stored: the SHA-256 of theta, swdown, lwdown and
cloud_cover OVER THE TILE after every call (`sha_call<n>_<field>`: equal hashes == 0 differing bits), of cloud_cover over the whole
rows jts..jte (the 5e-8 columns outside its:ite), the three 2-D results of every call in full, theta after the last call while it
fits FULL_BYTES, and the shares of the clips / branches taken in the first call as the CPU restatement flags them.  Only runs
where the reference is present; tests/test_ra_oracle.py pins the restatement to these files everywhere."""
import ctypes
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
import ra_oracle as R  # noqa: E402

FULL_BYTES = 200 * 1024


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402
MODULES = ["constants/icar_constants", "constants/wrf_constants", "utilities/time_delta_obj", "utilities/time_h", "main/data_structures",
           "objects/opt_types", "objects/options_h", "utilities/assertions", "objects/grid_h", "objects/meta_data_h", "objects/variable_h",
           "objects/variable_dict_h", "objects/exchangeable_h", "objects/boundary_h", "objects/domain_h", "physics/mp_thompson",
           "utilities/atm_utilities", "physics/ra_simple"]
TIME_SUB = """
submodule (time_object) ra_time_two
  implicit none
contains
  module function calc_day_of_year(this, lon)
    implicit none
    real                        :: calc_day_of_year
    class(Time_type), intent(in):: this
    real,             intent(in), optional :: lon
    real :: offset
    real(real128) :: year_start
    offset = 0
    if (present(lon)) then
      if (lon>180) then
        offset = (lon-360) / 360.0
      else
        offset = lon / 360.0
      endif
    endif
    year_start = 0
    calc_day_of_year = this%current_date_time - year_start + offset
  end function calc_day_of_year

  module function calc_year_fraction(this, lon)
    implicit none
    real                        :: calc_year_fraction
    class(Time_type)            :: this
    real, intent(in), optional  :: lon
    real :: offset
    real(real128) :: year_start, next_year_start
    offset = 0
    if (this%calendar==GREGORIAN) then
      year_start = 0
      next_year_start = this%year_zero
      if (present(lon)) then
        if (lon>180) then
          offset = (lon-360) / 360.0
        else
          offset = lon / 360.0
        endif
      endif
      calc_year_fraction = (this%current_date_time + offset - year_start) / (next_year_start - year_start)
    else if (this%calendar==NOLEAP) then
      calc_year_fraction = this%day_of_year(lon) / 365.0
    else if (this%calendar==THREESIXTY) then
      calc_year_fraction = this%day_of_year(lon) / 360.0
    endif
    calc_year_fraction = mod(calc_year_fraction, 1.0)
  end function calc_year_fraction
end submodule
"""
SHIM = """
module ra_shim
  use iso_c_binding
  use iso_fortran_env, only: real128
  use time_object,       only: Time_type
  use options_interface, only: options_t
  use data_structures
  use module_ra_simple, only: ra_simple, cos_lat_m, sin_lat_m, nrad_layers
  implicit none
  type(options_t), save :: options
contains
  subroutine ref_ra_simple(nx, nz, ny, theta, pii, qv, qc, qs, qi, qg, qr, p, swdown, lwdown, cloud_cover, lat, lon, &
                           days, year_days, calendar, dt, its, ite, jts, jte, kts, kte, runlw) bind(C, name="ref_ra_simple")
    integer(c_int), value :: nx, nz, ny, its, ite, jts, jte, kts, kte, runlw, calendar, year_days
    real(c_double), value :: days
    real(c_float), value :: dt
    real(c_float), dimension(nx,nz,ny) :: theta, pii, qv, qc, qs, qi, qg, qr, p
    real(c_float), dimension(nx,ny) :: swdown, lwdown, cloud_cover, lat, lon
    type(Time_type) :: date
    if (allocated(cos_lat_m)) deallocate(cos_lat_m)
    if (allocated(sin_lat_m)) deallocate(sin_lat_m)
    allocate(cos_lat_m(1:nx, 1:ny)); allocate(sin_lat_m(1:nx, 1:ny))
    cos_lat_m = cos(lat / 360.0 * 2*pi)          ! ra_simple_init, ra_simple.f90:75-78
    sin_lat_m = sin(lat / 360.0 * 2*pi)
    nrad_layers = 5
    date%calendar = calendar
    date%year_zero = year_days
    date%current_date_time = real(days, real128)
    call ra_simple(theta=theta, pii=pii, qv=qv, qc=qc, qs=qs + qi + qg, qr=qr, p=p, swdown=swdown, lwdown=lwdown, &
                   cloud_cover=cloud_cover, lat=lat, lon=lon, date=date, options=options, dt=dt, &
                   ims=1, ime=nx, jms=1, jme=ny, kms=1, kme=nz, its=its, ite=ite, jts=jts, jte=jte, kts=kts, kte=kte, &
                   F_runlw=(runlw /= 0))
  end subroutine
end module
"""


def build_reference(tmp):
    """libraref.so in tmp: the reference's modules where they lie, our shim + date submodule and the link stubs of oracle/ (see build_ref.sh)"""
    src = os.path.join(REF, "src")
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-fcoarray", "-w", "-DUSE_ASSERTIONS=.false.", "-I" + os.path.join(src, "physics"), "-I" + os.path.join(src, "utilities")]
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    run([FC, "-c", "-O2", "-fPIC", "-w", os.path.join(ROOT, "oracle", "ref_link_stubs.f90"), "-o", "ref_link_stubs.o"])
    run(["gcc", "-c", "-fPIC", os.path.join(ROOT, "oracle", "ref_link_stubs.c"), "-o", "ref_link_stubs_c.o"])
    objs = ["ref_link_stubs.o", "ref_link_stubs_c.o"]
    for m in MODULES:
        o = os.path.basename(m) + ".o"
        run([FC] + flags + [os.path.join(src, m + ".f90"), "-o", o])
        objs.append(o)
    for name, text in (("ra_time_two", TIME_SUB), ("ra_shim", SHIM)):
        open(os.path.join(tmp, name + ".f90"), "w").write(text)
        run([FC] + flags + [name + ".f90", "-o", name + ".o"])
        objs.append(name + ".o")
    # type-bound procedures of the interface modules whose bodies live in the uncompiled *_obj.f90 files: never called here
    und = subprocess.check_output(["nm", "-u"] + objs, cwd=tmp, text=True)
    dfn = subprocess.check_output(["nm", "--defined-only"] + objs, cwd=tmp, text=True)
    undef = {l.split()[1] for l in und.splitlines() if len(l.split()) == 2 and l.split()[0] == "U" and l.split()[1].startswith("_QM")}
    defined = {l.split()[2] for l in dfn.splitlines() if len(l.split()) == 3}
    open(os.path.join(tmp, "defsyms.rsp"), "w").write("\n".join(f"-Wl,--defsym,{s}=0" for s in sorted(undef - defined)))
    run([FC, "-shared", "-o", "libraref.so"] + objs + ["@defsyms.rsp"])
    return ctypes.CDLL(os.path.join(tmp, "libraref.so"))


def run_reference(L, c, A, n=0, tile=None, kts=1, kte=None, runlw=None):
    ny, nz, nx = c["pressure"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    D, yd = R.clock(c, n)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ci = ctypes.c_int
    L.ref_ra_simple(ci(nx), ci(nz), ci(ny), p(A["potential_temperature"]), *[p(c[k]) for k in R.INPUTS[1:]], p(A["shortwave"]), p(A["longwave"]),
                    p(A["cloud_fraction"]), p(c["latitude"]), p(c["longitude"]), ctypes.c_double(D), ci(int(yd)), ci(c["calendar"]),
                    ctypes.c_float(c["ra_dt"] * (n + 1)), ci(its), ci(ite), ci(jts), ci(jte), ci(kts), ci(nz if kte is None else kte),
                    ci(int(c["runlw"] if runlw is None else runlw)))


def differing(c, A, B, tile=None):
    """cells of the reference's state A and the restatement's B that differ where the reference's result is defined"""
    m, rows = R.tile_mask(c, tile)
    return {"potential_temperature": R.bitdiff(A["potential_temperature"], B["potential_temperature"]),
            "shortwave": R.bitdiff(A["shortwave"][m], B["shortwave"][m]),
            "longwave": R.bitdiff(A["longwave"][m], B["longwave"][m]),
            "cloud_fraction": R.bitdiff(A["cloud_fraction"], B["cloud_fraction"])}


def make(L, name):
    p = R.CASES[name]
    c = R.make_case(**p)
    m, rows = R.tile_mask(c)
    A = R.state(c); B = R.state(c)
    out = {"input_fingerprint": np.float64(R.fingerprint(c))}
    same = True
    for n in range(R.CALLS):
        run_reference(L, c, A, n)
        fl = R.run_oracle(c, B, n, flags=True)                      # (only for the recorded shares)
        if n == 0:
            cells = (fl & R.FLAGS["cell"]) != 0
            shares = {k: float(((fl & v) != 0)[cells].mean()) for k, v in R.FLAGS.items() if k != "cell"}
        same = same and not any(differing(c, A, B).values())
        out[f"sha_call{n + 1}_potential_temperature"] = np.array(sha(A["potential_temperature"]))
        for k in R.OUTPUTS[1:]:
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(A[k][m]))
            out[f"call{n + 1}_{k}"] = np.where(m | ((k == "cloud_fraction") & rows), A[k], np.float32(R.SENTINEL)).astype(np.float32)
        out[f"sha_call{n + 1}_cloud_fraction_rows"] = np.array(sha(A["cloud_fraction"][rows]))
    if A["potential_temperature"].nbytes <= FULL_BYTES:
        out[f"call{R.CALLS}_potential_temperature"] = A["potential_temperature"].copy()
    else:                                                           # as many of the lowest levels as fit
        nk = FULL_BYTES // (A["potential_temperature"][:, 0, :].nbytes)
        out[f"call{R.CALLS}_potential_temperature_lowest"] = A["potential_temperature"][:, :nk, :].copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), shares=np.array(json.dumps(shares)), **out)
    print("wrote", name, "restatement == reference:", same, {k: round(v, 3) for k, v in shares.items()})
    return same


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_ra: the reference sources are not present")
    with tempfile.TemporaryDirectory(prefix="icar_raref_") as tmp:
        L = build_reference(tmp)
        ok = [make(L, n) for n in (sys.argv[1:] or R.CASES)]
        sys.exit(0 if all(ok) else 1)

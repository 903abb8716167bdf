#!/usr/bin/env python
"""Golden vectors of the simple boundary-layer scheme under tests/golden/pbl_simple_*.npz made by RUNNING THE REFERENCE'S OWN
MODULE: src/physics/pbl_simple.f90 compiled unmodified (the flags and interface modules of oracle/build_ref.sh up to domain_h, then
physics/pbl_simple) together with the bind(C) shim below, in a temporary directory outside the repository; init_simple_pbl +
simple_pbl run CALLS times on each case of tests/pbl_oracle.py:CASES with the state carried from call to call.  Inputs are
regenerated from the recorded recipe (a fingerprint detects drift).  Stored: the SHA-256 of every scalar after every call
(`sha_call<n>_<field>`, over the REAL(4) bytes: equal hashes == 0 differing bits), the fields themselves after the last call for as
many scalars, in simple_pbl's argument order, as fit FULL_BYTES (a fixture stays well below the largest one of tests/golden/), the
rows' sub-step counts as the CPU restatement gives them and the shares of the clips / branches taken in the first call.  Only runs where the reference
is present; tests/test_pbl_oracle.py pins the restatement to these files everywhere."""
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
import pbl_oracle as P  # noqa: E402

FULL_BYTES = 400 * 1024


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402
MODULES = ["constants/icar_constants", "constants/wrf_constants", "utilities/time_delta_obj", "utilities/time_h", "main/data_structures",
           "objects/opt_types", "objects/options_h", "utilities/assertions", "objects/grid_h", "objects/meta_data_h", "objects/variable_h",
           "objects/variable_dict_h", "objects/exchangeable_h", "objects/boundary_h", "objects/domain_h", "physics/pbl_simple"]
SHIM = """
module pbl_shim
  use iso_c_binding
  use domain_interface,  only: domain_t
  use options_interface, only: options_t
  use pbl_simple, only: simple_pbl, init_simple_pbl, finalize_simple_pbl
  implicit none
  type(options_t), save :: options
  type(domain_t), allocatable, save :: domain
contains
  subroutine ref_pbl_simple(nx, nz, ny, th, qv, qc, qi, qr, qs, um, vm, pii, rho, z, dz, terrain, land_mask, &
                            its, ite, jts, jte, kts, kte, dt) bind(C, name="ref_pbl_simple")
    integer(c_int), value :: nx, nz, ny, its, ite, jts, jte, kts, kte
    real(c_float), value :: dt
    real(c_float), dimension(nx,nz,ny) :: th, qv, qc, qi, qr, qs, um, vm, pii, rho, z, dz
    real(c_float), dimension(nx,ny) :: terrain
    integer(c_int), dimension(nx,ny) :: land_mask
    if (.not.allocated(domain)) allocate(domain)
    domain%ims = 1; domain%ime = nx; domain%jms = 1; domain%jme = ny; domain%kms = 1; domain%kme = nz
    domain%ids = 1; domain%ide = nx; domain%jds = 1; domain%jde = ny; domain%kds = 1; domain%kde = nz
    call finalize_simple_pbl()
    call init_simple_pbl(domain, options)
    call simple_pbl(th, qv, qc, qi, qr, qs, um, vm, pii, rho, z, dz, terrain, land_mask, its, ite, jts, jte, kts, kte, dt)
  end subroutine
end module
"""


def build_reference(tmp):
    """libpblref.so in tmp: the reference's modules where they lie, our shim and the link stubs of oracle/ (see build_ref.sh)"""
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
    open(os.path.join(tmp, "pbl_shim.f90"), "w").write(SHIM)
    run([FC] + flags + ["pbl_shim.f90", "-o", "pbl_shim.o"])
    objs.append("pbl_shim.o")
    # type-bound procedures of the interface modules whose bodies live in the uncompiled *_obj.f90 files: never called here
    und = subprocess.check_output(["nm", "-u"] + objs, cwd=tmp, text=True)
    dfn = subprocess.check_output(["nm", "--defined-only"] + objs, cwd=tmp, text=True)
    undef = {l.split()[1] for l in und.splitlines() if len(l.split()) == 2 and l.split()[0] == "U" and l.split()[1].startswith("_QM")}
    defined = {l.split()[2] for l in dfn.splitlines() if len(l.split()) == 3}
    open(os.path.join(tmp, "defsyms.rsp"), "w").write("\n".join(f"-Wl,--defsym,{s}=0" for s in sorted(undef - defined)))
    run([FC, "-shared", "-o", "libpblref.so"] + objs + ["@defsyms.rsp"])
    return ctypes.CDLL(os.path.join(tmp, "libpblref.so"))


def run_reference(R, c, A, tile=None):
    ny, nz, nx = c["z"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ci = ctypes.c_int
    R.ref_pbl_simple(ci(nx), ci(nz), ci(ny), *[p(A[k]) for k in P.SCALARS], p(c["u_mass"]), p(c["v_mass"]), p(c["exner"]), p(c["density"]),
                     p(c["z"]), p(c["dz_mass"]), p(c["terrain"]), p(c["land_mask"]), ci(its), ci(ite), ci(jts), ci(jte), ci(1), ci(nz),
                     ctypes.c_float(c["pbl_dt"]))


def make(R, name):
    p = P.CASES[name]
    c = P.make_case(**p)
    A = P.state(c); B = P.state(c)
    out = {"input_fingerprint": np.float64(P.fingerprint(c))}
    nsubs = []
    for n in range(P.CALLS):
        run_reference(R, c, A)
        nsub, fl = P.run_oracle(c, B, flags=True)                   # (only for the recorded sub-step counts and shares)
        nsubs.append(nsub)
        if n == 0:
            cells = (fl & P.FLAGS["cell"]) != 0
            shares = {k: float(((fl & v) != 0)[cells].mean()) for k, v in P.FLAGS.items() if k != "cell"}
        for k in P.SCALARS:
            out[f"sha_call{n + 1}_{k}"] = np.array(sha(A[k]))
    room = FULL_BYTES
    for k in P.SCALARS:
        if A[k].nbytes <= room:
            out[f"call{P.CALLS}_{k}"] = A[k].copy(); room -= A[k].nbytes
    out["nsubsteps"] = np.stack(nsubs)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), shares=np.array(json.dumps(shares)), **out)
    same = all(np.array_equal(A[k].view(np.int32), B[k].view(np.int32)) for k in P.SCALARS)
    print("wrote", name, "nsubsteps", sorted(set(np.stack(nsubs)[:, 1:-1].ravel().tolist())), "restatement == reference:", same,
          {k: round(v, 3) for k, v in shares.items()})


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_pbl: the reference sources are not present")
    with tempfile.TemporaryDirectory(prefix="icar_pblref_") as tmp:
        R = build_reference(tmp)
        for n in (sys.argv[1:] or P.CASES):
            make(R, n)

#!/usr/bin/env python
"""Golden vectors of the Tiedtke convection scheme under tests/golden/cu_tiedtke_*.npz made by RUNNING THE REFERENCE'S OWN CODE:
src/physics/cu_tiedtke.f90 WHOLE AND UNMODIFIED, compiled with the flang of oracle/build_ref.sh in a temporary directory outside the
repository, behind a bind(C) shim of our own (below) that calls CU_TIEDTKE with the arguments of src/physics/cu_driver.f90:303-330
(itimestep = STEPCU = 1, the levels kts .. kte-1, every F_Q* flag true, QFX / HFX given).  Nothing of the reference is written.

Every case of tests/tiedtke_oracle.py:CASES runs CALLS carried calls; the second call's state has the first call's tendencies
applied.  Stored per call: the four tendencies, RAINCV and PRATEC in full.  Before anything is written the generator asserts
  (0) tests/support/tiedtke_oracle.c (the product's icar_amd/csrc/tiedtke_column.h) reproduces the compiled reference bit for bit in
      RTHCUTEN, RQVCUTEN, RQCCUTEN, RQICUTEN, RAINCV and PRATEC, for every case and the further seeds of SEEDS;
  (a) the reference itself gives every column the same bits with each row's columns other than the first reversed, and one column
      per call with the row's first column kept first (so the early exits shared along a row change no column);
  (b) the reference with other U3D / V3D, other QFX and other HFX changes nothing but RUCUTEN / RVCUTEN (the winds are passive, and
      the surface fluxes are read only by a comparison that PQTE = 0 decides);
  (d) the coverage conditions of COVER hold, each in one fixture for at least 2 % of its columns and at least 4 columns.
(c) of the issue -- an interface within 50 hPa of 300 hPa in every column -- guards KTOP0, which only the KTYPE = 1 closure reads;
with itimestep = 1 no column is ever of KTYPE 1 (see the header), so there is nothing for it to guard.
Only runs where the reference is present; tests/test_tiedtke_oracle.py pins the restatement to these files everywhere."""
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
import tiedtke_oracle as T  # noqa: E402

REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402

SHIM = """
module tiedtke_shim
  use iso_c_binding
  use module_cu_tiedtke
  implicit none
contains
  subroutine ref_cu_tiedtke(nx, nz, ny, its, ite, jts, jte, kte, dt, qfx, hfx, znu, u, v, w, t, qv, qc, qi, pii, rho, dz, pmid, pint, xland, &
                            raincv, pratec, tth, tqv, tqc, tqi, tu, tv) bind(C, name="ref_cu_tiedtke")
    integer(c_int), value :: nx, nz, ny, its, ite, jts, jte, kte
    real(c_float), value :: dt
    real(c_float), dimension(nx,ny) :: qfx, hfx, xland, raincv, pratec
    real(c_float), dimension(nz) :: znu
    real(c_float), dimension(nx,nz,ny) :: u, v, w, t, qv, qc, qi, pii, rho, dz, pmid, pint, tth, tqv, tqc, tqi, tu, tv
    real, allocatable, dimension(:,:,:) :: qv_adv, qv_pbl
    logical, allocatable, dimension(:,:) :: flag
    allocate(qv_adv(nx,nz,ny)); allocate(qv_pbl(nx,nz,ny)); allocate(flag(nx,ny))
    qv_adv = 0; qv_pbl = 0; flag = .false.
    call CU_TIEDTKE(dt, 1, 1, raincv, pratec, qfx, hfx, znu, u, v, w, t, qv, qc, qi, pii, rho, qv_adv, qv_pbl, dz, pmid, pint, xland, flag, &
                    1, nx+1, 1, ny+1, 1, nz+1, 1, nx, 1, ny, 1, nz, its, ite, jts, jte, 1, kte-1, tth, tqv, tqc, tqi, tu, tv, &
                    .True., .True., .True., .True., .True.)
  end subroutine
end module
"""

RES = T.TEND + T.OUT2
# name -> (what it is, a function of (diag flags, A) giving a boolean mask over the tile's columns)
COVER = {
    "midlevel":   ("KTYPE = 3 started by CUBASMC, a cloud above it", lambda d, A: (d & T.D_MIDLEVEL != 0) & (A["ktype"] == 3)),
    "precip":     ("convection with surface precipitation", lambda d, A: (A["ktype"] == 3) & (A["raincv"] > 0)),
    "none":       ("no convection", lambda d, A: A["ktype"] == 0),
    "downdraft":  ("a downdraft (LODDRAF)", lambda d, A: d & T.D_DOWNDRAFT != 0),
    "melting":    ("melting (ZDPMEL /= 0)", lambda d, A: d & T.D_MELT != 0),
    "evaporation": ("rain evaporating below cloud base in CUFLX", lambda d, A: d & T.D_EVAP != 0),
    "pcte_warm":  ("PCTE > 0, ZTPP1 >= t000", lambda d, A: d & T.D_PCTE_WARM != 0),
    "pcte_cold":  ("PCTE > 0, ZTPP1 <= hgfr", lambda d, A: d & T.D_PCTE_COLD != 0),
    "pcte_mixed": ("PCTE > 0, in between (exp evaluated)", lambda d, A: d & T.D_PCTE_MIXED != 0),
    "mfmax":      ("the cloud-base mass flux cut to ZMFMAX", lambda d, A: d & T.D_MFMAX != 0),
    "ice":        ("TLUCUA's ice arm", lambda d, A: d & T.D_ICE != 0),
    "liquid":     ("TLUCUA's water arm", lambda d, A: d & T.D_WATER != 0),
    "land":       ("lndj = 1", lambda d, A: A["lndj"] == 1),
    "water":      ("lndj = 0", lambda d, A: A["lndj"] == 0),
}
SHARE = {"none": 0.20}


def build_reference(tmp):
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-w"]
    run([FC] + flags + [os.path.join(REF, "src", "physics", "cu_tiedtke.f90"), "-o", "cu_tiedtke.o"])
    open(os.path.join(tmp, "tiedtke_shim.f90"), "w").write(SHIM)
    run([FC] + flags + ["tiedtke_shim.f90", "-o", "tiedtke_shim.o"])
    run([FC, "-shared", "-o", "libtiedtkeref.so", "cu_tiedtke.o", "tiedtke_shim.o"])
    return ctypes.CDLL(os.path.join(tmp, "libtiedtkeref.so"))


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def ref_call(L, c, A, dt, tile=None, wind=None, qfx=None, hfx=None, sel=None):
    """CU_TIEDTKE of the reference on the tile; sel: index array along i -- the call then sees those columns only, in that order,
    as a domain of its own (one row of columns per j), and the results are scattered back"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = tile or T.tile_of(c)
    rng = np.random.default_rng(11)
    u, v = wind if wind is not None else (rng.normal(0, 8, (ny, nz, nx)).astype(np.float32), rng.normal(0, 8, (ny, nz, nx)).astype(np.float32))
    qfx = np.full((ny, nx), 2e-5, np.float32) if qfx is None else qfx
    hfx = np.full((ny, nx), 40.0, np.float32) if hfx is None else hfx
    names3 = {"u": u, "v": v, "w": c["w_real"], "t": A["temperature"], "qv": A["water_vapor"], "qc": A["cloud_water"], "qi": A["cloud_ice"],
              "pi": c["exner"], "rho": c["density"], "dz": c["dz_interface"], "p": c["pressure"], "pint": c["pressure_interface"]}
    names2 = {"qfx": qfx, "hfx": hfx, "xland": c["xland"]}
    if sel is not None:
        names3 = {k: np.ascontiguousarray(a[:, :, sel]) for k, a in names3.items()}
        names2 = {k: np.ascontiguousarray(a[:, sel]) for k, a in names2.items()}
        nxs, its, ite = len(sel), 1, len(sel)
    else:
        nxs = nx
    out3 = {k: np.zeros((ny, nz, nxs), np.float32) for k in T.TEND + ["tend_u", "tend_v"]}
    out2 = {k: np.zeros((ny, nxs), np.float32) for k in T.OUT2}
    ci = ctypes.c_int
    L.ref_cu_tiedtke(ci(nxs), ci(nz), ci(ny), ci(its), ci(ite), ci(jts), ci(jte), ci(nz), ctypes.c_float(dt), _p(names2["qfx"]), _p(names2["hfx"]),
                     _p(c["znu"]), *[_p(names3[k]) for k in ("u", "v", "w", "t", "qv", "qc", "qi", "pi", "rho", "dz", "p", "pint")],
                     _p(names2["xland"]), _p(out2["raincv"]), _p(out2["pratec"]), *[_p(out3[k]) for k in T.TEND + ["tend_u", "tend_v"]])
    out3.update(out2)
    return out3


def same(c, X, Y, keys=RES, tile=None):
    return {k: T.bitdiff(T.owned(c, X[k], tile), T.owned(c, Y[k], tile)) for k in keys}


def check_rows(L, c, A, dt, R):
    """(a): permuted rows and single columns against the whole-row run R"""
    ny, nz, nx = c["density"].shape
    its, ite, jts, jte = T.tile_of(c)
    first = its - 1
    rest = np.arange(its, ite)
    sel = np.concatenate([[first], rest[::-1]])
    P = ref_call(L, c, A, dt, sel=sel)
    for k in RES:
        assert T.bitdiff(P[k][jts - 1:jte], R[k][jts - 1:jte][..., sel]) == 0, f"(a) a row's columns reversed change {k}"
    for i in rest[:: max(1, len(rest) // 6)]:                                 # one column per call behind the row's leveltop column
        sel = np.array([first, i])
        S = ref_call(L, c, A, dt, sel=sel)
        for k in RES:
            assert T.bitdiff(S[k][jts - 1:jte], R[k][jts - 1:jte][..., sel]) == 0, f"(a) column {i} alone differs in {k}"


def check_passive(L, c, A, dt, R):
    """(b)"""
    ny, nz, nx = c["density"].shape
    rng = np.random.default_rng(12)
    W = ref_call(L, c, A, dt, wind=(rng.normal(5, 20, (ny, nz, nx)).astype(np.float32), rng.normal(-3, 20, (ny, nz, nx)).astype(np.float32)),
                 qfx=rng.uniform(-1e-4, 4e-4, (ny, nx)).astype(np.float32), hfx=rng.uniform(-100, 600, (ny, nx)).astype(np.float32))
    d = same(c, W, R)
    assert not any(d.values()), f"(b) other winds and surface fluxes change {d}"


def make(L, name, p, write=True, cover=None):
    c = T.make_case(**p)
    A, O = T.state(c), T.state(c)
    out = {"input_fingerprint": np.float64(T.fingerprint(c))}
    ok = True
    its, ite, jts, jte = T.tile_of(c)
    for n in range(T.CALLS):
        if n:
            T.carry(c, A, T.DT[n - 1])
        R = ref_call(L, c, A, T.DT[n])
        T.run_oracle(c, O, n)
        for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature"):
            assert T.bitdiff(A[k], O[k]) == 0
        d = same(c, R, O)
        ok = ok and not any(d.values())
        if any(d.values()):
            print("   call", n + 1, "differing bits:", {k: v for k, v in d.items() if v})
        for k in RES:
            assert np.isfinite(R[k]).all(), f"{name}: the reference's {k} is not finite after call {n + 1}"
            assert T.bitdiff(R[k], O[k]) == 0 or not ok, f"{name}: {k} written outside the tile"
            A[k] = R[k]
            out[f"call{n + 1}_{k}"] = R[k].copy()
        check_rows(L, c, A, T.DT[n], R)
        check_passive(L, c, A, T.DT[n], R)
        dg = T.owned(c, O["diag"])
        Ao = {"ktype": T.owned(c, O["ktype"]), "raincv": T.owned(c, O["raincv"]),
              "lndj": np.abs(T.owned(c, c["xland"]) - 2).astype(np.int32)}
        if cover is not None:
            for k, (_, f) in COVER.items():
                m = f(dg, Ao)
                cover.setdefault(k, []).append((name, n + 1, int(m.sum()), int(m.size)))
    lt = [(T.leveltop(c, its, j), sorted({T.leveltop(c, i, j) for i in range(its, ite + 1)})) for j in range(jts, jte + 1)]
    out["leveltop"] = np.array([a for a, _ in lt], np.int32)
    if p.get("terrain"):
        assert len({a for a, _ in lt}) > 1, f"{name}: leveltop is the same in every row"
        assert any(len(b) > 1 for _, b in lt), f"{name}: every column of a row gives the same leveltop"
        if "lid" in p and p["lid"] < 10000.0:                                    # ... and which column is first changes results
            X, Y = T.state(c), T.state(c)
            T.cu_tiedtke(c, X, T.DT[0]); T.cu_tiedtke(c, Y, T.DT[0], leveltop_col=ite)
            assert T.bitdiff(T.owned(c, X["tend_th"]), T.owned(c, Y["tend_th"])) > 0, f"{name}: leveltop from another column changes nothing"
    print(name, "restatement == reference:", ok, "leveltop", sorted({a for a, _ in lt}))
    if write and ok:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), **out)
    return ok


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_tiedtke: the reference sources are not present")
    write = "--dry" not in sys.argv
    with tempfile.TemporaryDirectory(prefix="icar_tdkref_") as tmp:
        L = build_reference(tmp)
        cover = {}
        res = [make(L, n, p, False, cover) for n, p in T.CASES.items()]
        res += [make(L, n, p, False, None) for n, p in T.SEEDS.items()]
        good = all(res)
        for k, rows in cover.items():
            best = max(rows, key=lambda r: r[2] / r[3])
            need = max(4, int(np.ceil(SHARE.get(k, 0.02) * best[3])))
            print(f"  coverage {k:12s} {COVER[k][0]:50s} best {best[2]:4d} of {best[3]:4d} ({best[0]} call {best[1]}), needs {need}")
            if best[2] < need:
                good = False
                print("    NOT MET")
        if good and write:
            for n, p in T.CASES.items():
                make(L, n, p, True, None)
        sys.exit(0 if good else 1)

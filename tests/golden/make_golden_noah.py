#!/usr/bin/env python
"""Golden vectors of the Noah land-surface model under tests/golden/noah_*.npz made by RUNNING THE REFERENCE'S OWN CODE:
src/physics/lsm_noahlsm.f90 and src/physics/lsm_noahdrv.f90 WHOLE AND UNMODIFIED, compiled with the flang and the flags of
oracle/build_ref.sh in a temporary directory outside the repository, behind a bind(C) shim of our own (below).  The three .TBL files
of the reference's run/ are copied there; LSM_NOAH_INIT is called with the arguments of src/physics/lsm_driver.f90:677-705 (so it
calls SOIL_VEG_GEN_PARM("MODIFIED_IGBP_MODIS_NOAH", "STAS") itself) and lsm_noah with those of :1210-1278 and the constants of
allocate_noah_data (:425-520).  Nothing of the reference is written, neither its text nor its tables' files: noah_tables.npz holds the
tables AS THE REFERENCE PARSED THEM, read from the module's public variables.

Every case of tests/noah_oracle.py:CASES runs its carried calls (four to six); only the forcing changes between them.  Stored per
call: every array lsm_noah writes (noah_oracle.OUT), and the arrays after lsm_init.  Before anything is written the generator asserts
  (0) tests/support/noah_oracle.c (the product's icar_amd/csrc/noah_column.h) reproduces the compiled reference bit for bit in every
      output, for every case and the further seeds of SEEDS -- except, on LAND-ICE cells, the arrays of noah_oracle.ICE_UNSET: there
      the reference stores locals that only SFLX sets (noah_column.h), i.e. what the cell before left; (d) below shows it;
  (a) the reference itself gives the same bits when a call is repeated after an unrelated call;
  (b) the reference gives every cell the same bits with each row reversed;
  (c) single cells computed alone have the bits they have in the tile;
      (a) .. (c) over every output on land and water cells and over the defined outputs on land-ice cells;
  (d) at least one ICE_UNSET value of a land-ice cell DOES change when the row is reversed or the cell computed alone;
  (e) every stored output is finite (the ICE_UNSET values of land-ice cells are stored as the restatement leaves them: unchanged);
  (f) the coverage conditions of COVER, each in some fixture and call for at least 2 % of the cells that run SFLX there; every fixture
      has at least 20 % such cells, 5 % water cells and one land-ice cell; the two CYCLES (snow falls and later melts, soil freezes
      and later thaws, in the same cell over the carried calls of one fixture) likewise; the conditions of ABSENT and NOT_REACHED
      never hold.
The flags of (f) come from the restatement and count only once (0) holds.
Only runs where the reference is present; tests/test_noah_oracle.py pins the restatement to these files everywhere."""
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
import noah_oracle as N  # noqa: E402

REF = os.environ.get("ICAR_REFERENCE", "/root/reference")
from icar_amd.build import FLANG as FC  # noqa: E402

f32 = np.float32
# lsm_noah's array arguments in the order the shim takes them
REF3 = ["dz8w", "qv3d", "p8w3d", "t3d"]
REF2 = ["tsk", "hfx", "qfx", "lh", "grdflx", "qgh", "gsw", "swdown", "glw", "smstav", "smstot", "sfcrunoff", "udrunoff", "vegfra", "albedo",
        "albbck", "znt", "z0", "tmn", "xland", "xice", "emiss", "embck", "snowc", "qsfc", "rainbl", "snow", "canwat", "chs", "chs2", "cqs2",
        "cpm", "sr", "chklowq", "lai", "qz0", "snowh", "snoalb", "shdmin", "shdmax", "snotime", "acsnom", "acsnow", "snopcx", "potevp", "rib",
        "noahres", "flx4", "fvb", "fbur", "fgsn"]
REFS = ["smois", "tslb", "sh2o", "smcrel"]

SHIM = """
module noah_shim
  use iso_c_binding
  use module_sf_noahdrv
  use module_sf_noahlsm
  implicit none
contains
  subroutine ref_noah_init(nx, ny, its, ite, jts, jte, fnd, vegfra, snow, snowc, snowh, canwat, sfcrunoff, udrunoff, acsnow, acsnom, &
                           ivgtyp, isltyp, tslb, smois, sh2o, snoalb) bind(C, name="ref_noah_init")
    integer(c_int), value :: nx, ny, its, ite, jts, jte, fnd
    real(c_float), dimension(nx,ny) :: vegfra, snow, snowc, snowh, canwat, sfcrunoff, udrunoff, acsnow, acsnom, snoalb
    integer(c_int), dimension(nx,ny) :: ivgtyp, isltyp
    real(c_float), dimension(nx,4,ny) :: tslb, smois, sh2o
    real :: zs(4), dzs(4)
    integer :: i
    logical :: fndsnowh
    fndsnowh = fnd /= 0
    dzs = [0.1,0.3,0.6,1.0]
    zs(1) = dzs(1)/2
    do i = 2,4
        zs(i) = zs(i-1) + dzs(i)/2 + dzs(i-1)/2
    end do
    call LSM_NOAH_INIT(vegfra, snow, snowc, snowh, canwat, tslb, smois, sfcrunoff, udrunoff, acsnow, acsnom, ivgtyp, isltyp, tslb, smois, &
                       sh2o, zs, dzs, "MODIFIED_IGBP_MODIS_NOAH", snoalb, .false., fndsnowh, .false., 4, .false., .true., &
                       1, nx+1, 1, ny+1, 1, 3, 1, nx, 1, ny, 1, 2, its, ite, jts, jte, 1, 2)
  end subroutine
  subroutine ref_noah_tables(iv, fv, fs, fsl, gen, ints) bind(C, name="ref_noah_tables")
    integer(c_int) :: iv(NLUS), ints(4)
    real(c_float) :: fv(NLUS,13), fs(NSLTYPE,10), fsl(NSLOPE), gen(13)
    iv = NROTBL
    fv(:,1) = SNUPTBL; fv(:,2) = RSTBL; fv(:,3) = RGLTBL; fv(:,4) = HSTBL; fv(:,5) = MAXALB; fv(:,6) = EMISSMINTBL; fv(:,7) = EMISSMAXTBL
    fv(:,8) = LAIMINTBL; fv(:,9) = LAIMAXTBL; fv(:,10) = Z0MINTBL; fv(:,11) = Z0MAXTBL; fv(:,12) = ALBEDOMINTBL; fv(:,13) = ALBEDOMAXTBL
    fs(:,1) = BB; fs(:,2) = DRYSMC; fs(:,3) = F11; fs(:,4) = MAXSMC; fs(:,5) = REFSMC; fs(:,6) = SATPSI; fs(:,7) = SATDK; fs(:,8) = SATDW
    fs(:,9) = WLTSMC; fs(:,10) = QTZ
    fsl = SLOPE_DATA
    gen = [TOPT_DATA, CMCMAX_DATA, CFACTR_DATA, RSMAX_DATA, SBETA_DATA, FXEXP_DATA, CSOIL_DATA, SALP_DATA, REFDK_DATA, REFKDT_DATA, &
           FRZK_DATA, ZBOT_DATA, LVCOEF_DATA]
    ints = [BARE, LUCATS, SLCATS, SLPCATS]
  end subroutine
  subroutine ref_lsm_noah(nx, ny, its, ite, jts, jte, dt, isurban, isice, ivgtyp, isltyp, %(args)s) bind(C, name="ref_lsm_noah")
    integer(c_int), value :: nx, ny, its, ite, jts, jte, isurban, isice
    real(c_float), value :: dt
    integer(c_int), dimension(nx,ny) :: ivgtyp, isltyp
    real(c_float), dimension(nx,2,ny) :: %(a3)s
    real(c_float), dimension(nx,ny) :: %(a2)s
    real(c_float), dimension(nx,4,ny) :: %(as)s
    real :: dzs(4)
    dzs = [0.1,0.3,0.6,1.0]
    call lsm_noah(dz8w, qv3d, p8w3d, t3d, tsk, hfx, qfx, lh, grdflx, qgh, gsw, swdown, glw, smstav, smstot, sfcrunoff, udrunoff, ivgtyp, isltyp, &
                  isurban, isice, vegfra, albedo, albbck, znt, z0, tmn, xland, xice, emiss, embck, snowc, qsfc, rainbl, &
                  "MODIFIED_IGBP_MODIS_NOAH", 4, dt, dzs, 1, smois, tslb, snow, canwat, chs, chs2, cqs2, cpm, 287.058/1003.5, sr, chklowq, lai, &
                  qz0, .false., .false., sh2o, snowh, snoalb, shdmin, shdmax, snotime, acsnom, acsnow, snopcx, potevp, smcrel, 1.0, .false., &
                  .false., rib, noahres, .false., flx4, fvb, fbur, fgsn, 1, nx+1, 1, ny+1, 1, 3, 1, nx, 1, ny, 1, 2, its, ite, jts, jte, 1, 2)
  end subroutine
end module
"""


def wrap(names):
    out, line = [], ""
    for n in names:
        if len(line) + len(n) > 100:
            out.append(line + " &\n        ")
            line = ""
        line += n + ", "
    return ("".join(out) + line).rstrip(", ")


cond = lambda name: (lambda d, c: d & N.D[name] != 0)
# name -> (what it is, a mask over the tile's cells from (flags, case))
COVER = {
    "nopac":          ("NOPAC: no snow on the ground", cond("NOPAC")),
    "snopac_melt":    ("SNOPAC with melt (SNOMLT > 0)", cond("SNOPAC_MELT")),
    "snopac_nomelt":  ("SNOPAC without melt", cond("SNOPAC_NOMELT")),
    "new_snow":       ("new snow (FFROZP = 1, PRCP > 0) through SNOW_NEW", cond("NEW_SNOW")),
    "rain_bare":      ("rain on bare ground (SHDFAC = 0)", cond("RAIN_BARE")),
    "rain_veg":       ("rain on vegetated ground", cond("RAIN_VEG")),
    "drip":           ("canopy drip (EXCESS > CMCMAX)", cond("DRIP")),
    "dew":            ("dew (ETP < 0)", cond("DEW")),
    "canres":         ("CANRES called (SHDFAC > 0)", cond("CANRES")),
    "no_canres":      ("CANRES not called", cond("NO_CANRES")),
    "smflx_two":      ("SMFLX's two-pass arm", cond("SMFLX_TWO")),
    "smflx_one":      ("SMFLX's one-pass arm", cond("SMFLX_ONE")),
    "srt_frozen":     ("SRT with frozen ground (DICE > 1.E-2)", cond("SRT_FROZEN")),
    "frh2o_iter":     ("FRH2O's iteration converging", cond("FRH2O_ITER")),
    "snksrc_pos":     ("SNKSRC > 0: freezing", cond("SNKSRC_POS")),
    "snksrc_neg":     ("SNKSRC < 0: thawing", cond("SNKSRC_NEG")),
    "tdfcnd_frozen":  ("TDFCND's frozen arm", cond("TDFCND_FROZEN")),
    "tdfcnd_unfrozen": ("TDFCND's unfrozen arm", cond("TDFCND_UNFROZEN")),
    "snfrac_below":   ("SNFRAC below SNUP", cond("SNFRAC_BELOW")),
    "snfrac_full":    ("SNFRAC at or above SNUP", cond("SNFRAC_FULL")),
    "snowh_rederived": ("SNOWH <= SNEQV: re-derived (:804)", cond("SNOWH_REDERIVED")),
    "snow_warm":      ("T1 > 273.14 with snow (:749-752)", cond("SNOW_WARM")),
    "snow_cold":      ("the cold arm with snow (:753-757)", cond("SNOW_COLD")),
    "soil14":         ("SOILTYP = 14 on land reset to 7", cond("SOIL14")),
    "urban":          ("VEGTYP == ISURBAN", cond("URBAN")),
    "sstep_max":      ("SSTEP's clip at SMCMAX: runoff from an over-full layer", cond("SSTEP_MAX")),
    "sstep_min":      ("SSTEP's clips at 0.02 and at 0", cond("SSTEP_MIN")),
    "frzgra":         ("freezing rain", cond("FRZGRA")),
}
# excluded by the call (DESIGN 3.8 says why): asserted absent
ABSENT = ["VEG25_27"]
# not reached by any case or seed with physical inputs (DESIGN 3.8 says what was tried): asserted absent from the fixtures, so that a
# recipe that does reach one is noticed and the condition moved to COVER
NOT_REACHED = ["FRH2O_FALLBACK", "FRH2O_BADLOG"]
# over the carried calls of one fixture
CYCLES = {"snow_cycle": ("snow falls (SNOW_NEW) and melts in a later call", "NEW_SNOW", "SNOPAC_MELT"),
          "soil_cycle": ("soil freezes (SNKSRC > 0) and thaws in a later call", "SNKSRC_POS", "SNKSRC_NEG")}


def build_reference(tmp):
    run = lambda cmd: subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    flags = ["-c", "-cpp", "-O2", "-fPIC", "-fcoarray", "-w"]
    run([FC, "-c", "-O2", "-fPIC", "-w", os.path.join(ROOT, "oracle", "ref_link_stubs.f90"), "-o", "ref_link_stubs.o"])
    run(["gcc", "-c", "-fPIC", os.path.join(ROOT, "oracle", "ref_link_stubs.c"), "-o", "ref_link_stubs_c.o"])
    run([FC] + flags + [os.path.join(REF, "src", "physics", "lsm_noahlsm.f90"), "-o", "lsm_noahlsm.o"])
    run([FC] + flags + [os.path.join(REF, "src", "physics", "lsm_noahdrv.f90"), "-o", "lsm_noahdrv.o"])
    open(os.path.join(tmp, "noah_shim.f90"), "w").write(SHIM % dict(args=wrap(REF3 + REF2 + REFS), a3=wrap(REF3), a2=wrap(REF2), **{"as": wrap(REFS)}))
    run([FC] + flags + ["noah_shim.f90", "-o", "noah_shim.o"])
    run([FC, "-shared", "-o", "libnoahref.so", "lsm_noahlsm.o", "lsm_noahdrv.o", "noah_shim.o", "ref_link_stubs.o", "ref_link_stubs_c.o"])
    for t in ("VEGPARM.TBL", "SOILPARM.TBL", "GENPARM.TBL"):
        shutil.copy(os.path.join(REF, "run", t), tmp)
    return ctypes.CDLL(os.path.join(tmp, "libnoahref.so"))


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
ci, cf = ctypes.c_int, ctypes.c_float


def quiet(f, *a):
    """the reference prints from LSM_NOAH_INIT and FRH2O: its standard output goes nowhere while it runs"""
    sys.stdout.flush()
    keep, null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        return f(*a)
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)


def sub(a, rows, cols):
    return np.ascontiguousarray(a[rows][..., cols])


def ref_init(L, tmp, c, A, rows=None, cols=None):
    """LSM_NOAH_INIT of the reference as lsm_init calls it (:672-707) on the cells rows x cols as a domain of their own; A is written"""
    rows = np.arange(c["ny"]) if rows is None else rows
    cols = np.arange(c["nx"]) if cols is None else cols
    names = ["vegfra", "snow", "snowc", "snowh", "canwat", "sfcrunoff", "udrunoff", "acsnow", "acsnom", "ivgtyp", "isltyp", "tslb", "smois", "sh2o", "snoalb"]
    S = {k: sub(c[k] if k in c else A[k], rows, cols) for k in names}
    keep = S["canwat"].copy()
    here = os.getcwd()
    os.chdir(tmp)
    try:
        quiet(L.ref_noah_init, ci(len(cols)), ci(len(rows)), ci(1), ci(len(cols)), ci(1), ci(len(rows)), ci(int(c["fndsnowh"])), *[_p(S[k]) for k in names])
    finally:
        os.chdir(here)
    S["canwat"] = keep                                                            # lsm_driver.f90:672, :707
    return S


def tables(L):
    iv, ints = np.zeros(N.NLUS, np.int32), np.zeros(4, np.int32)
    fv, fs = np.zeros((13, N.NLUS), f32), np.zeros((10, N.NSLTYPE), f32)
    fsl, gen = np.zeros(N.NSLOPE, f32), np.zeros(13, f32)
    L.ref_noah_tables(_p(iv), _p(fv), _p(fs), _p(fsl), _p(gen), _p(ints))
    tab = {"nrotbl": iv, "slope_data": fsl}
    tab.update({k: fv[i].copy() for i, k in enumerate(N.T_VEG)})
    tab.update({k: fs[i].copy() for i, k in enumerate(N.T_SOIL)})
    tab.update({k: gen[i] for i, k in enumerate(N.T_GEN)})
    tab.update({k: ints[i] for i, k in enumerate(N.T_INT)})
    return tab


def ref_call(L, c, A, n, rows=None, cols=None):
    """lsm_noah of the reference with the forcing of call n on the cells rows x cols, in that order, as a domain of their own; the
    outputs come back in that order and A is left alone"""
    rows = np.arange(c["ny"]) if rows is None else rows
    cols = np.arange(c["nx"]) if cols is None else cols
    ny, nx = len(rows), len(cols)
    F = c["forcing"][n]
    zero = np.zeros((ny, nx), f32)
    S = {}
    for k in REF2 + REFS + ["ivgtyp", "isltyp"]:
        src = F.get(k, c.get(k, A.get(k)))
        S[k] = sub(src, rows, cols).copy() if src is not None else zero.copy()
    S["embck"] = np.full((ny, nx), 0.99, f32)
    two = lambda a, b: np.ascontiguousarray(np.stack([sub(a, rows, cols), sub(b, rows, cols)], axis=1))
    S["dz8w"] = np.full((ny, 2, nx), 40.0, f32)
    S["qv3d"] = two(F["qv"], F["qv"])
    S["p8w3d"] = two(F["p8w1"], F["p8w2"])
    S["t3d"] = two(F["t"], F["t"])
    quiet(L.ref_lsm_noah, ci(nx), ci(ny), ci(1), ci(nx), ci(1), ci(ny), cf(float(c["dt"])), ci(N.ISURBAN), ci(N.ISICE), _p(S["ivgtyp"]), _p(S["isltyp"]),
          *[_p(S[k]) for k in REF3 + REF2 + REFS])
    return S


def diffs(c, X, Y, rows=None, cols=None, keys=N.OUT):
    """differing bits per output; the ICE_UNSET arrays are compared outside the land-ice cells only"""
    rows = np.arange(c["ny"]) if rows is None else rows
    cols = np.arange(c["nx"]) if cols is None else cols
    ice = sub(N.ice_cells(c), rows, cols)
    out = {}
    for k in keys:
        x, y = X[k].view(np.uint32), np.ascontiguousarray(Y[k], f32).view(np.uint32)
        ne = x != y
        if k in N.ICE_UNSET:
            ne = ne & ~ice
        out[k] = int(ne.sum())
    return out


def unset_diffs(c, X, Y, rows, cols):
    ice = sub(N.ice_cells(c), rows, cols)
    return sum(int(((X[k].view(np.uint32) != np.ascontiguousarray(Y[k], f32).view(np.uint32)) & ice).sum()) for k in N.ICE_UNSET)


def make(L, tmp, tab, name, p, write=True, cover=None, other=None):
    c = N.make_case(tab, **p)
    A, O = N.state0(c), N.state0(c)
    out = {"input_fingerprint": np.float64(N.fingerprint(c))}
    ok = True
    S = ref_init(L, tmp, c, A)
    N.lsm_init(tab, c, O)
    for k in ("sh2o", "snoalb", "snowh", "canwat"):
        A[k] = S[k]
        d = N.bitdiff(A[k], O[k])
        ok = ok and d == 0
        if d:
            print("   lsm_init differing bits in", k, d)
        assert np.isfinite(A[k]).all()
        out["init_" + k] = A[k].copy()
    i0, j0 = c["nx"] // 2, c["ny"] // 2                                               # LSM_NOAH_INIT on a single cell and a reversed row
    S1 = ref_init(L, tmp, c, N.state0(c), np.array([j0]), np.arange(c["nx"])[::-1])
    assert all(N.bitdiff(S1[k], sub(A[k], np.array([j0]), np.arange(c["nx"])[::-1])) == 0 for k in ("sh2o", "snoalb", "snowh")), "(b) init"
    ice = N.ice_cells(c)
    land = (c["xland"] < 1.5) & ~ice
    assert ice.any() and (c["xland"] > 1.5).mean() >= 0.05 and land.mean() >= 0.2, name
    unset_seen, hist = 0, []
    allrows, allcols = np.arange(c["ny"]), np.arange(c["nx"])
    for n in range(N.ncalls(p)):
        R = ref_call(L, c, A, n)
        N.lsm_noah(tab, c, O, n)
        d = diffs(c, R, O)
        ok = ok and not any(d.values())
        if any(d.values()):
            print("   call", n + 1, "differing bits:", {k: v for k, v in d.items() if v})
        if other:                                                                      # (a)
            oc, oA = other
            ref_call(L, oc, oA, 0)
            R2 = ref_call(L, c, A, n)
            assert not any(diffs(c, R, R2).values()), f"(a) {name}: a repeated call gives other bits"
        rev = allcols[::-1]                                                            # (b)
        P = ref_call(L, c, A, n, allrows, rev)
        Rr = {k: sub(R[k], allrows, rev) for k in N.OUT}
        assert not any(diffs(c, P, Rr, allrows, rev).values()), f"(b) {name}: a row reversed changes a cell"
        unset_seen += unset_diffs(c, P, Rr, allrows, rev)
        cells = [(j, i) for j in range(c["ny"]) for i in range(c["nx"])]                # (c)
        for j, i in cells[:: max(1, len(cells) // 40)] + list(zip(*np.nonzero(ice))):
            rj, ri = np.array([j]), np.array([i])
            S1 = ref_call(L, c, A, n, rj, ri)
            R1 = {k: sub(R[k], rj, ri) for k in N.OUT}
            assert not any(diffs(c, S1, R1, rj, ri).values()), f"(c) {name}: cell {i},{j} alone differs from its bits in the tile"
            unset_seen += unset_diffs(c, S1, R1, rj, ri)
        for k in N.ICE_UNSET:                                                          # stored as the restatement leaves them
            R[k][ice] = O[k][ice]
        for k in N.OUT:
            assert np.isfinite(R[k]).all(), f"(e) {name}: the reference's {k} is not finite after call {n + 1}"
            A[k] = R[k]
            out[f"call{n + 1}_{k}"] = R[k].copy()
        if cover is not None:
            dg = O["diag"]
            ran = dg & N.D["SFLX"] != 0
            assert ran.mean() >= 0.2
            for k, (_, f) in COVER.items():
                cover.setdefault(k, []).append((name, n + 1, int((f(dg, c) & ran).sum()), int(ran.sum())))
            for k in ABSENT + NOT_REACHED:
                assert not (dg & N.D[k]).any(), f"{name}: {k} was reached"
            hist.append(dg.copy())
    if cover is not None:
        ran = hist[-1] & N.D["SFLX"] != 0
        for k, (_, first, then) in CYCLES.items():
            m = np.zeros(ran.shape, bool)
            for a in range(len(hist)):
                for b in range(a + 1, len(hist)):
                    m |= (hist[a] & N.D[first] != 0) & (hist[b] & N.D[then] != 0)
            cover.setdefault(k, []).append((name, len(hist), int(m.sum()), int(ran.sum())))
    assert unset_seen, f"(d) {name}: no unset value of a land-ice cell ever depended on the cell before"
    print(name, "restatement == reference:", ok, " land-ice values that depend on the cell before:", unset_seen)
    if write and ok:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), params=np.array(json.dumps(p)), **out)
    return ok


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("make_golden_noah: the reference sources are not present")
    write = "--dry" not in sys.argv
    with tempfile.TemporaryDirectory(prefix="icar_noahref_") as tmp:
        L = build_reference(tmp)
        first = N.make_case({"maxsmc": np.full(N.NSLTYPE, 0.4), "wltsmc": np.full(N.NSLTYPE, 0.1)}, nx=5, ny=4, seed=99, dt=600.0, t=[280.0], sw=[100],
                            pr=[(0.5, 1.0)], snow0=0.2)
        ref_init(L, tmp, first, N.state0(first))                                        # reads the three tables
        tab = tables(L)
        assert int(tab["lucats"]) == 21 and int(tab["slcats"]) == 19 and int(tab["bare"]) == 16
        oc = N.make_case(tab, nx=9, ny=7, seed=98, dt=900.0, t=[275.0], sw=[300], pr=[(0.5, 2.0)], snow0=0.3)
        oA = N.state0(oc)
        N.lsm_init(tab, oc, oA)
        other = (oc, oA)
        cover = {}
        res = [make(L, tmp, tab, n, p, False, cover, other) for n, p in N.CASES.items()]
        res += [make(L, tmp, tab, n, p, False, None, other) for n, p in N.SEEDS.items()]
        good = all(res)
        for k, rows in cover.items():
            best = max(rows, key=lambda r: r[2] / max(r[3], 1))
            need = max(2, int(np.ceil(0.02 * best[3])))
            print(f"  coverage {k:16s} {(COVER.get(k) or CYCLES[k])[0]:56s} best {best[2]:4d} of {best[3]:4d} ({best[0]} call {best[1]}), needs {need}")
            if best[2] < need:
                good = False
                print("    NOT MET")
        if good and write:
            np.savez_compressed(N.TABLES, **tab)
            for n, p in N.CASES.items():
                make(L, tmp, tab, n, p, True, None, other)
        sys.exit(0 if good else 1)

"""The CPU restatement of the boundary-layer slot with kPBL_YSU (tests/support/ysu_oracle.c: the product's cell and column header
compiled for the host) against the vectors of the compiled reference (tests/golden/ysu_*.npz, tests/golden/make_golden_ysu.py):
pbl_init's arrays and, after each of the two carried calls, every result, exch_h and the six tendencies as ysu leaves them and the
four updated fields, 0 differing bits; the conditions that keep the fixtures honest; the two further seeds against the reference
compiled on the spot where its sources are present.  CPU only.

Which cells count for which condition.  Each condition must hold after some call of SOME fixture.  regime, Ri and kpbl are taken from
the REFERENCE's vectors; what ysu2d keeps in locals (pblflg, the branch a half level took, the clips) is taken from the restatement's
own flags (ysu_column.h: YSU_D_*, YSU_C_*), which the bit-for-bit comparison of every result ties to the reference.
  unstable / stable           Ri <= 0 / Ri > 0, columns of the tile                                   each >= 20 % in one fixture
  da_sfc_wtq's regimes        regime = 1.1, 2.1, 3.1, 4.1, cells of the MEMORY (da_sfc_wtq runs over it)   each >= 2 %
  the boundary-layer top      pblflg columns of the tile: kpbl takes >= 4 distinct values; kpbl = 1 in >= 5 % of the tile's columns
  moist diffusion (:897), ri < 0 (:910)          half levels of the tile at or above kpbl (k = kpbl .. kte-1)       >= 1 % on each side
  entrainment (entfac < 4.6, :984)               those half levels in pblflg columns                              >= 1 % on each side
  xkzmin, xkzmax, prmax                          all half levels of the tile (below and above kpbl)               >= 1 % on each side
  gamcrt, gamcrq                                 unstable (sfcflg) columns of the tile                            >= 1 % on each side
  rimin                                          columns of the tile                                              >= 1 % on each side
  prmin                                          CANNOT be taken: below kpbl prnum >= phih/phim + bfac karman sfcfrac > 0.2788 > prmin, at
                                                 and above kpbl prnum = 1 + 2.1 ri >= 1; asserted never taken
and one fixture each with the minimum level count, 64 and 90 levels, -0.0 cells in cloud water (inside the tile, in the halo column of
an owned row and in a halo row at the top level), all land, >= 30 % water, and >= 1 % of the cells at the 1e-5 floor of the wind speed."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import ysu_oracle as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
REF = os.environ.get("ICAR_REFERENCE", "/root/reference")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def replay(name):
    c = Y.make_case(**Y.CASES[name])
    A = Y.state(c)
    init = {k: A[k].copy() for k in Y.INIT2}
    states = []
    for n in range(Y.CALLS):
        keep = {}
        Y.run_oracle(c, A, n, keep=keep)
        s = {k: A[k].copy() for k in Y.STATE3 + Y.OUT2 + ["exch_h"]}
        s.update(keep)
        s["zero"] = not any(A[k].any() for k in Y.TEND)
        states.append(s)
    return c, init, states


@pytest.fixture(scope="module")
def replays():
    return {n: replay(n) for n in Y.CASES}


@pytest.mark.parametrize("name", list(Y.CASES))
def test_restatement_equals_reference_vectors(replays, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert json.loads(str(z["params"])) == Y.CASES[name]
    c, init, states = replays[name]
    assert float(z["input_fingerprint"]) == Y.fingerprint(c), "the recipe's inputs drifted: rerun tests/golden/make_golden_ysu.py"
    for k in Y.INIT2:
        assert Y.bitdiff(init[k], z["init_" + k]) == 0, (name, k)
    assert (z["init_zol"] == 10).all() and (z["init_hol"] == 1000).all()
    for n in range(Y.CALLS):
        s = states[n]
        for k in Y.OUT2 + ["exch_h", "tend_th", "tend_qv", "tend_qc", "tend_qi"]:
            assert Y.bitdiff(s[k], z[f"call{n + 1}_{k}"]) == 0, (name, n + 1, k, Y.bitdiff(s[k], z[f"call{n + 1}_{k}"]))
            assert np.isfinite(s[k]).all()
        for k in ("tend_u", "tend_v") + tuple(Y.STATE3):
            assert sha(s[k]) == str(z[f"sha_call{n + 1}_{k}"]), f"{name}: {k} of call {n + 1} differs from the compiled reference"
        assert s["zero"], "the six tendencies are zero behind pbl"
        # ysu leaves the top model level and everything outside the tile without a tendency
        its, ite, jts, jte = Y.tile_of(c)
        out = np.ones(c["water_vapor"].shape, bool); out[jts - 1:jte, :-1, its - 1:ite] = False
        for k in Y.TEND:
            assert not s[k][out].any(), (name, k)
        assert (s["tend_th"] != 0).any() and (s["tend_qv"] != 0).any()
    for k in ("tend_u", "tend_v", "cloud_water"):
        assert Y.bitdiff(states[-1][k], z[f"call{Y.CALLS}_{k}"]) == 0, (name, k)


def test_fixture_conditions(replays):
    covs, floors, cases = [], [], []
    seen = dict(minimum=False, lev64=False, lev90=False, negzero=False)
    for name in Y.CASES:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        c, init, states = replays[name]
        stored = json.loads(str(z["coverage"]))
        for n in range(Y.CALLS):
            A = {k: z[f"call{n + 1}_{k}"] for k in ("ri", "kpbl", "regime")}           # the reference's own results
            cv = Y.coverage(c, A, {"diag": states[n]["diag"]})
            assert cv == stored[n], (name, n + 1)
            covs.append(cv)
        floors.append(float((z["call1_windspd"] == np.float32(1e-5)).mean()))
        calm = (c["u_10m"] == 0) & (c["v_10m"] == 0)
        assert np.array_equal(z["call1_windspd"] == np.float32(1e-5), calm)
        cases.append(c)
        ny, nz, nx = c["z"].shape
        seen["minimum"] |= nz == Y.MIN_NZ() == 3
        seen["lev64"] |= nz == 64
        seen["lev90"] |= nz == 90
        if c["negzero"]:
            qc0, qc2 = c["cloud_water"], z[f"call{Y.CALLS}_cloud_water"]
            neg = np.signbit(qc0) & (qc0 == 0)
            its, ite, jts, jte = Y.tile_of(c)
            assert neg[jts - 1:jte, :, its - 1:ite].any() and neg[jts - 1:jte, :, 0].any() and neg[0, -1, :].any(), "inside the tile, halo column, halo row at the top"
            assert not np.signbit(qc2[neg]).any(), "x + tend dt with tend = 0 over the whole memory: -0.0 becomes +0.0"
            seen["negzero"] = True
    import make_golden_ysu as G
    assert G.holds(covs, floors, cases) == []
    assert all(seen.values()), seen


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not present")
def test_further_seeds_against_the_compiled_reference(tmp_path_factory):
    import make_golden_ysu as G
    L, forms = G.build_reference(str(tmp_path_factory.mktemp("ysuref")))
    assert forms == G.EXPECTED_POW, "the compiled reference keeps other powers as calls than ysu_column.h states"
    for name, p in Y.EXTRA_SEEDS.items():
        same, out, covs, floor, c = G.make(L, name, p)
        assert same, name

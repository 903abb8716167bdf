"""The CPU restatement of the Noah branch of lsm() (tests/support/lsm_noah_driver_oracle.c: the product's lsm_noah_driver_cell.h around
noah_column.h) against the vectors of the compiled reference under tests/golden/lsm_noah_*.npz (tests/golden/make_golden_lsm_noah.py):
after lsm_init and after every carried call, in every array the block writes, 0 differing bits; the gates; the coverage shares,
recomputed here; the FMA-contracted build of the restatement differs, as it should.  Where the reference is present the two unstored
seeds run through the generator's own build of it as well."""
import json
import os
import sys

import numpy as np
import pytest

import lsm_noah_driver_oracle as LN
import noah_oracle as N
from util import equals_reference_vector

GOLDEN = LN.GOLDEN


@pytest.fixture(scope="module")
def tab():
    return N.load_tables()


def run(tab, name, contract=False):
    """the restatement over the fixture's calls: [(state after lsm_init)], [(state after call n)], gates, flags"""
    c = LN.make_case(tab, **LN.CASES[name])
    L = LN.lib(contract=contract)
    A = LN.state0(c)
    LN.lsm_init(tab, c, A, L)
    init = {k: A[k].copy() for k in LN.INIT + ["sh2o", "snoalb", "snowh", "canwat"]}
    calls, gates, flags = [], [], []
    for n in range(len(c["forcing"])):
        is_open, pf, qf = LN.lsm(tab, c, A, n, None, L)
        gates.append(is_open)
        if is_open:
            flags.append((pf, qf))
        calls.append({k: A[k].copy() for k in N.OUT + LN.DRV})
    return c, init, calls, gates, flags


@pytest.mark.parametrize("name", list(LN.CASES))
def test_restatement_equals_the_reference_vectors(tab, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c, init, calls, gates, flags = run(tab, name)
    assert float(z["input_fingerprint"]) == LN.fingerprint(c), "the recipe of the case changed: regenerate the fixture"
    its, ite, jts, jte = LN.tile_of(c)
    t2, t3 = (slice(jts - 1, jte), slice(its - 1, ite)), (slice(jts - 1, jte), slice(None), slice(its - 1, ite))
    cut = lambda a, k: np.ascontiguousarray(a[t3 if a.ndim == 3 else t2]) if k not in LN.DRV + LN.WHOLE + LN.INIT else a
    for k in LN.INIT + ["sh2o", "snoalb", "snowh", "canwat"]:                      # LSM_NOAH_INIT ran on the reference's tile
        assert equals_reference_vector(cut(init[k], k), cut(z["init_" + k], k)), f"{name}: {k} after lsm_init"
    assert list(z["gates"]) == gates and gates.count(False) == 1
    for n, got in enumerate(calls):
        for k in N.OUT + LN.DRV:
            assert equals_reference_vector(cut(got[k], k), cut(z[f"call{n + 1}_{k}"], k)), f"{name}, call {n + 1}: {k}"
    assert json.loads(str(z["shares"])) == LN.shares(c, flags)
    ice = N.ice_cells(c)
    assert 0 < ice.mean() <= 0.05, "land ice stays at or below 5 % of a fixture's cells"


def test_coverage(tab):
    """each arm in at least 2 % of the tile's cells of some fixture; what cannot be reached never occurs (README, round 22, says why)"""
    best = {}
    for name in LN.CASES:
        c, _, _, _, flags = run(tab, name)
        for k, v in LN.shares(c, flags).items():
            best[k] = max(best.get(k, 0.0), v)
    for k in LN.REQUIRED:
        assert best[k] >= 0.02, (k, best[k])
    assert best["wind0"] >= 1
    for k in LN.NOT_REACHED:
        assert best[k] == 0.0, f"{k} was reached: move it to REQUIRED"


def test_fma_contracted_restatement_differs(tab):
    """the compiled reference has no contraction on this path: a contracted build of the same text gives other bits"""
    name = "lsm_noah_a_snowfall_melt_24x12"
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert bool(z["fma_contracted_differs"])
    _, _, calls, _, _ = run(tab, name, contract=True)
    assert any(LN.bitdiff(calls[-1][k], z[f"call{len(calls)}_{k}"]) for k in ("rib", "chs", "lwup", "t2", "q2"))


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get("ICAR_REFERENCE", "/root/reference"), "src")), reason="the reference sources are not present")
def test_unstored_seeds_through_the_compiled_reference(tab, tmp_path):
    sys.path.insert(0, GOLDEN)
    import make_golden_lsm_noah as M
    L = M.build_reference(str(tmp_path))
    first = N.make_case({"maxsmc": np.full(N.NSLTYPE, 0.4), "wltsmc": np.full(N.NSLTYPE, 0.1)}, nx=5, ny=4, seed=99, dt=600.0, t=[280.0], sw=[100],
                        pr=[(0.5, 1.0)], snow0=0.2)
    M.G.ref_init(L, str(tmp_path), first, N.state0(first))                          # reads the three tables
    for name, p in LN.SEEDS.items():
        ok, fma = M.make(L, str(tmp_path), tab, name, p, False, None)
        assert ok and fma, name

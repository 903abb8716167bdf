"""The CPU restatement of the simple boundary-layer scheme (tests/support/pbl_oracle.c) against the vectors of the compiled
reference (tests/golden/pbl_simple_*.npz, tests/golden/make_golden_pbl.py): every scalar after every one of the three carried calls,
0 differing bits (SHA-256 of the REAL(4) bytes; the stored fields of the last call are also compared cell by cell), and the
coverage conditions that keep the fixtures honest -- no fixture set passes without exercising every clip and branch of the
scheme and the whole range of sub-step counts.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import pbl_oracle as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def replay(name):
    """the restatement over the three calls of a case: states after every call, sub-step counts, flags of the first call"""
    c = P.make_case(**P.CASES[name])
    A = P.state(c)
    states, nsubs, flags = [], [], None
    for n in range(P.CALLS):
        nsub, fl = P.run_oracle(c, A, flags=True)
        if n == 0: flags = fl
        states.append({k: A[k].copy() for k in P.SCALARS}); nsubs.append(nsub)
    return c, states, np.stack(nsubs), flags


@pytest.fixture(scope="module")
def replays():
    return {n: replay(n) for n in P.CASES}


@pytest.mark.parametrize("name", list(P.CASES))
def test_restatement_equals_reference_vectors(replays, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert json.loads(str(z["params"])) == P.CASES[name]
    c, states, nsubs, _ = replays[name]
    assert float(z["input_fingerprint"]) == P.fingerprint(c), "the recipe's inputs drifted: rerun tests/golden/make_golden_pbl.py"
    stored = 0
    for n in range(P.CALLS):
        for k in P.SCALARS:
            assert sha(states[n][k]) == str(z[f"sha_call{n + 1}_{k}"]), f"{name}: {k} after call {n + 1} differs from the compiled reference"
            key = f"call{n + 1}_{k}"
            if key in z.files:
                stored += 1
                assert P.bitdiff(states[n][k], z[key]) == 0, (name, key, P.bitdiff(states[n][k], z[key]))
            assert np.isfinite(states[n][k]).all()
    assert stored >= 2
    assert np.array_equal(nsubs, z["nsubsteps"])
    assert not np.array_equal(states[-1]["potential_temperature"], c["potential_temperature"]), "the scheme must have done something"


def test_fixtures_cover_the_scheme(replays):
    """The conditions of the issue that no set of fixtures can pass without exercising the scheme."""
    seen = set()
    best = {k: 0.0 for k in P.FLAGS if k != "cell"}
    for name, (c, states, nsubs, fl) in replays.items():
        rows = nsubs[:, 1:-1]                                           # the rows jts..jte of the tile
        seen |= set(rows.ravel().tolist())
        if "calm" not in name:
            assert (rows > 1).any() and (rows == 1).any(), f"{name}: rows with and without sub-stepping"
        else:
            assert (rows == 1).all()
        cells = (fl & P.FLAGS["cell"]) != 0
        ny, nz, nx = fl.shape
        assert int(cells.sum()) == (nx - 2) * (ny - 2) * (nz - 1)
        for k in best:
            best[k] = max(best[k], float(((fl & P.FLAGS[k]) != 0)[cells].mean()))
    assert 1 in seen and 20 in seen and len([n for n in seen if 2 <= n <= 19]) >= 2, sorted(seen)
    assert max(seen) <= 21 and min(seen) >= 1
    for k, share in best.items():
        assert share >= 0.01, f"{k}: taken in {share:.4f} of the half-level cells of the best fixture (1 % asked)"


def test_restatement_refuses_an_empty_level_range():
    c = P.make_case(8, 6, 3, seed=9, rough=1.0, dt=30.0)
    with pytest.raises(ValueError):
        P.run_oracle(c, P.state(c), kts=3, kte=3)                       # kte is lowered to nz - 1 = 2 < kts


@pytest.mark.parametrize("seed", [101, 102])
def test_restatement_equals_fresh_reference_run(seed, tmp_path):
    """where the reference's sources are present: pbl_simple.f90 compiled now (the generator's recipe) on two further seeds, sub-tile
    and shortened level range included"""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden_pbl as G
    if not os.path.isdir(os.path.join(G.REF, "src")) or not os.path.exists(G.FC):
        pytest.skip("the reference sources (or flang) are not present on this host")
    R = G.build_reference(str(tmp_path))
    c = P.make_case(28, 16, 18 if seed == 101 else 5, seed=seed, rough=15.0, dt=100.0, th_noise=1.0)
    A, B = P.state(c), P.state(c)
    tile = (3, 20, 2, 11) if seed == 101 else None
    for n in range(3):
        G.run_reference(R, c, A, tile=tile)
        nsub, _ = P.run_oracle(c, B, tile=tile)
        for k in P.SCALARS:
            assert P.bitdiff(A[k], B[k]) == 0, (seed, n, k, P.bitdiff(A[k], B[k]))
    assert len(set(nsub.tolist())) > 2

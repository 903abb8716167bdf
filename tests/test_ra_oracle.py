"""The CPU restatement of the simple radiation scheme (tests/support/ra_oracle.c) against the vectors of the compiled reference
(tests/golden/ra_simple_*.npz, tests/golden/make_golden_ra.py): theta, swdown, lwdown and cloud_cover over the tile after every one
of the three carried calls, 0 differing bits (SHA-256 of the REAL(4) bytes; the stored fields are also compared cell by cell),
cloud_cover's 5e-8 columns outside its:ite, and the coverage conditions that keep the fixtures honest -- every clip and branch of
the scheme is taken in at least 1 % of the tile columns of one fixture and not taken in at least 1 % of one.  CPU only.

Two of the nine conditions are read as "the value sits AT its bound": `where(rh > 1) rh = 1` (:248) and `where(cloudfrac > 1)`
(:144) can never fire -- every term of the rh mean is already clipped to <= 1 by relative_humidity and a sum of five such
REAL(4) terms divided by 5 cannot round past 1; cloudfrac is a product of two factors <= 1 -- so the flags record rh == 1 and
cloudfrac == 1 after the clip."""
import hashlib
import json
import os

import numpy as np
import pytest

import ra_oracle as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def replay(name):
    """the restatement over the three calls of a case: states after every call, flags of the first call"""
    c = R.make_case(**R.CASES[name])
    A = R.state(c)
    states, flags = [], None
    for n in range(R.CALLS):
        fl = R.run_oracle(c, A, n, flags=True)
        if n == 0: flags = fl
        states.append({k: A[k].copy() for k in R.OUTPUTS})
    return c, states, flags


@pytest.fixture(scope="module")
def replays():
    return {n: replay(n) for n in R.CASES}


def shares_of(fl):
    cells = (fl & R.FLAGS["cell"]) != 0
    return {k: float(((fl & v) != 0)[cells].mean()) for k, v in R.FLAGS.items() if k != "cell"}, int(cells.sum())


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_reference_vectors(replays, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert json.loads(str(z["params"])) == R.CASES[name]
    c, states, fl = replays[name]
    assert float(z["input_fingerprint"]) == R.fingerprint(c), "the recipe's inputs drifted: rerun tests/golden/make_golden_ra.py"
    m, rows = R.tile_mask(c)
    for n in range(R.CALLS):
        s = states[n]
        assert sha(s["potential_temperature"]) == str(z[f"sha_call{n + 1}_potential_temperature"]), f"{name}: theta after call {n + 1} differs from the compiled reference"
        for k in R.OUTPUTS[1:]:
            assert sha(s[k][m]) == str(z[f"sha_call{n + 1}_{k}"]), f"{name}: {k} after call {n + 1} differs from the compiled reference"
            keep = m | rows if k == "cloud_fraction" else m
            assert R.bitdiff(s[k][keep], z[f"call{n + 1}_{k}"][keep]) == 0, (name, n + 1, k)
            assert np.isfinite(s[k][keep]).all()
        assert sha(s["cloud_fraction"][rows]) == str(z[f"sha_call{n + 1}_cloud_fraction_rows"])
        assert (s["cloud_fraction"][rows & ~m] == np.float32(5e-8)).all(), "cloud_cover outside its:ite on the rows jts..jte is 5e-8"
        assert (s["cloud_fraction"][~rows] == np.float32(R.SENTINEL)).all() and (s["shortwave"][~m] == np.float32(R.SENTINEL)).all()
    key = f"call{R.CALLS}_potential_temperature"
    if key in z.files:
        assert R.bitdiff(states[-1]["potential_temperature"], z[key]) == 0
    else:
        low = z[key + "_lowest"]
        assert R.bitdiff(states[-1]["potential_temperature"][:, :low.shape[1], :], low) == 0
    if c["runlw"]:
        assert not np.array_equal(states[-1]["potential_temperature"], c["potential_temperature"]), "the scheme must have cooled theta"
        assert (states[-1]["longwave"][m] > 100).all()
    else:
        assert np.array_equal(states[-1]["potential_temperature"], c["potential_temperature"]) and (states[-1]["longwave"] == np.float32(R.SENTINEL)).all()
    stored = json.loads(str(z["shares"]))
    mine, _ = shares_of(fl)
    assert stored == mine


def test_fixtures_cover_the_scheme(replays):
    """The conditions of the issue that no set of fixtures can pass without exercising the scheme."""
    taken = {k: 0.0 for k in R.FLAGS if k != "cell"}
    not_taken = dict(taken)
    calendars, crossed, norunlw = set(), False, False
    for name, (c, states, fl) in replays.items():
        sh, ncells = shares_of(fl)
        ny, nz, nx = c["pressure"].shape
        assert ncells == (nx - 2) * (ny - 2)
        for k, v in sh.items():
            taken[k] = max(taken[k], v); not_taken[k] = max(not_taken[k], 1.0 - v)
        calendars.add(c["calendar"]); norunlw |= not c["runlw"]
        crossed |= R.clock(c, 0)[1] != R.clock(c, R.CALLS - 1)[1] or R.clock(c, R.CALLS - 1)[0] < R.clock(c, 0)[0]
        assert abs(float(c["latitude"].max())) == 90.0 and float(c["latitude"].min()) == -90.0
        assert float(c["longitude"].min()) < -170 and float(c["longitude"].max()) > 350
    for k in taken:
        assert taken[k] >= 0.01, f"{k}: taken in {taken[k]:.4f} of the tile columns of the best fixture (1 % asked)"
        assert not_taken[k] >= 0.01, f"{k}: not taken in {not_taken[k]:.4f} of the tile columns of the best fixture (1 % asked)"
    assert calendars == {R.GREGORIAN, R.NOLEAP, R.THREESIXTY} and crossed and norunlw
    assert min(R.CASES[n]["nz"] for n in R.CASES) == 5 and len(R.CASES) >= 5


def test_day_night_and_sunrise_hours_are_covered(replays):
    sun = np.concatenate([s["shortwave"][R.tile_mask(c)[0]] for c, states, _ in replays.values() for s in states])
    assert (sun == 0).mean() > 0.05 and (sun > 300).mean() > 0.05 and ((sun > 0) & (sun < 30)).mean() > 0.005, "night, day and the hours next to sunrise"


@pytest.mark.parametrize("seed", [101, 102])
def test_restatement_equals_fresh_reference_run(seed, tmp_path):
    """where the reference's sources are present: ra_simple.f90 compiled now (the generator's recipe) on two further seeds, sub-tile
    and shortened level range included"""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden_ra as G
    if not os.path.isdir(os.path.join(G.REF, "src")) or not os.path.exists(G.FC):
        pytest.skip("the reference sources (or flang) are not present on this host")
    L = G.build_reference(str(tmp_path))
    c = R.make_case(28, 16, 18 if seed == 101 else 6, seed=seed, calendar=R.GREGORIAN if seed == 101 else R.NOLEAP, D0=100.3 if seed == 101 else 364.99,
                    advance=7200.0, dt=75.0)
    A, B = R.state(c), R.state(c)
    tile = (3, 20, 2, 11) if seed == 101 else None
    kts, kte = (2, 15) if seed == 101 else (1, None)
    for n in range(3):
        G.run_reference(L, c, A, n, tile=tile, kts=kts, kte=kte)
        R.run_oracle(c, B, n, tile=tile, kts=kts, kte=kte)
        assert not any(G.differing(c, A, B, tile).values()), (seed, n, G.differing(c, A, B, tile))

"""The CPU restatement of the surface-flux slot (tests/support/sfc_oracle.c) against the vectors of the compiled reference
(tests/golden/sfc_basic_*.npz, tests/golden/make_golden_sfc.py): every carried field after every one of the three carried calls, 0
differing bits (SHA-256 of the REAL(4) bytes; the stored fields are also compared cell by cell), the gate open, shut, open, and the
coverage conditions that keep the fixtures honest -- every branch of the slot is taken in at least 1 % of the relevant cells of one
fixture and not taken in at least 1 % of one.  CPU only.

"Relevant cells": for the ice / liquid coefficients of sat_mr, its p - e_s <= 0 clip, the sign of Ri and the ustar floor the open-water
cells of the memory interior; for wind == 0 every cell of the memory rectangle; for land / water the memory interior; for the two
clamps of layer_fraction the tile's cells on the levels kts+1 .. kts+nz; for the vapour floor the tile's cells of the loop ("in the
layer") and every cell at least two levels above the loop's last ("far above").  max(0, .) can fire only with kts > 1: with kts = 1 a
column's sum of dz below level k <= nz+1 is at most the sum of the levels' maxima, which is below sfc_layer_thickness by the
definition of nz -- the fixture with kts = 2 is there for it."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import sfc_oracle as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
FIELDS = S.STATE3 + S.STATE2


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def replay(name):
    """the restatement over the three calls of a case: states after every call, gates, flags of the first call"""
    c = S.make_case(**S.CASES[name])
    A = S.state(c)
    states, gates, flags = [], [], None
    for n in range(S.CALLS):
        is_open, wf, af = S.run_oracle(c, A, n, flags=True)
        if n == 0: flags = (wf, af)
        gates.append(is_open)
        states.append({k: A[k].copy() for k in FIELDS})
    return c, states, gates, flags


@pytest.fixture(scope="module")
def replays():
    return {n: replay(n) for n in S.CASES}


@pytest.mark.parametrize("name", list(S.CASES))
def test_restatement_equals_reference_vectors(replays, name):
    import make_golden_sfc as G
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert json.loads(str(z["params"])) == S.CASES[name]
    c, states, gates, (wf, af) = replays[name]
    assert float(z["input_fingerprint"]) == S.fingerprint(c), "the recipe's inputs drifted: rerun tests/golden/make_golden_sfc.py"
    assert gates == [bool(g) for g in z["gates"]] and int(z["layers"]) == S.layers(c, c["kts"])
    for n in range(S.CALLS):
        s = states[n]
        for k in FIELDS:
            assert sha(s[k]) == str(z[f"sha_call{n + 1}_{k}"]), f"{name}: {k} after call {n + 1} differs from the compiled reference"
            assert np.isfinite(s[k]).all()
        for k in S.STATE2:
            assert S.bitdiff(s[k], z[f"call{n + 1}_{k}"]) == 0, (name, n + 1, k)
        for k in S.STATE3:
            low = z[f"call{n + 1}_{k}_lowest"]
            assert S.bitdiff(s[k][:, :low.shape[1], :], low) == 0, (name, n + 1, k)
    assert json.loads(str(z["shares"])) == G.shares(c, wf, af)
    # the slot did something: theta and qv moved inside the tile's surface layer and nowhere else but at the floor
    moved = states[-1]["potential_temperature"] != c["potential_temperature"]
    assert moved.any() and not moved[:, c["kts"] + int(z["layers"]):, :].any() and not moved[0].any() and not moved[:, :, 0].any()
    assert (states[-1]["water_vapor"] >= np.float32(1e-10)).all()


def test_fixtures_cover_the_slot(replays):
    """The conditions of the issue that no set of fixtures can pass without exercising the slot."""
    import make_golden_sfc as G
    keys = ("water", "wind0", "ice", "clip", "ri_neg", "ustar_floor", "min1", "max0", "floor_layer", "floor_above")
    taken = {k: 0.0 for k in keys}
    not_taken = dict(taken)
    seen_gates, kts_seen, water_seen, deep = set(), set(), set(), 0
    for name, (c, states, gates, (wf, af)) in replays.items():
        sh = G.shares(c, wf, af)
        for k in keys:
            relevant = not (k in ("ice", "clip", "ri_neg", "ustar_floor", "water") and c["watersurface"] != S.kWATER_SIMPLE)
            relevant = relevant and not (k in ("min1", "max0") and S.layers(c, c["kts"]) == 0)
            if relevant:
                taken[k] = max(taken[k], sh[k]); not_taken[k] = max(not_taken[k], 1.0 - sh[k])
        seen_gates.add(tuple(gates)); kts_seen.add(c["kts"]); water_seen.add(c["watersurface"])
        deep = max(deep, S.layers(c, c["kts"]) - c["kts"] + 1)
        # dt varies from call to call, roughness_z0 is carried from water_simple into the next 10 m diagnostics
        if c["watersurface"] == S.kWATER_SIMPLE:
            assert S.bitdiff(states[0]["roughness_z0"], c["roughness_z0"]) > 0 and S.bitdiff(states[1]["u_10m"], states[0]["u_10m"]) > 0
    for k in keys:
        assert taken[k] >= 0.01, f"{k}: taken in {taken[k]:.4f} of the relevant cells of the best fixture (1 % asked)"
        assert not_taken[k] >= 0.01, f"{k}: not taken in {not_taken[k]:.4f} of the relevant cells of the best fixture (1 % asked)"
    assert (True, False, True) in seen_gates and kts_seen >= {1, 2} and water_seen == {0, 1, 2}
    assert deep >= 3 and len(S.CASES) >= 5 and S.CALLS == 3, "at least three levels inside the surface layer, five cases, three carried calls"


def test_plain_and_compensated_sums_differ_on_the_fixtures(replays):
    """the fixtures settle how sum(dz(i,kts:k-1,j)) is formed: the three candidate forms give different bits on them"""
    name = "sfc_basic_a_40x36x12"
    c = replays[name][0]
    out = []
    for mode in (0, 1, 2):
        A = S.state(c)
        S.apply_fluxes(c, A, 60.0, sum_mode=mode)
        out.append(A["water_vapor"])
    assert S.bitdiff(out[0], out[1]) > 0 and S.bitdiff(out[0], out[2]) > 0
    assert S.SUM_MODE == 0


def test_layer_past_kte_is_refused():
    c = S.make_case(10, 8, 4, seed=9)                                  # four levels of ~40-60 m: all of them below 400 m
    assert S.layers(c) == 4
    with pytest.raises(ValueError, match="reaches past kte"):
        S.apply_fluxes(c, S.state(c), 60.0)
    c = S.make_case(10, 8, 4, seed=9, thick=80.0)
    S.apply_fluxes(c, S.state(c), 60.0)


@pytest.mark.parametrize("seed", [101, 102])
def test_restatement_equals_fresh_reference_run(seed, tmp_path):
    """where the reference's sources are present: its statements compiled now (the generator's recipe) on two further seeds, a
    sub-tile and kts = 2 included"""
    import make_golden_sfc as G
    if not os.path.isdir(os.path.join(G.REF, "src")) or not os.path.exists(G.FC):
        pytest.skip("the reference sources (or flang) are not present on this host")
    L = G.load(G.build_reference(str(tmp_path)))
    c = S.make_case(28, 16, 11 if seed == 101 else 7, seed=seed, thick=400.0 if seed == 101 else 130.0, dt=75.0, kts=1 if seed == 101 else 2,
                    update_interval=300 if seed == 101 else 90)
    A, B = S.state(c), S.state(c)
    tile = (3, 20, 2, 11) if seed == 101 else None
    for n in range(3):
        G.run_reference(L, c, A, n, tile=tile)
        S.run_oracle(c, B, n, tile=tile)
        assert not any(G.differing(A, B).values()), (seed, n, G.differing(A, B))

"""The CPU restatement of the convection slot (tests/support/bmj_oracle.c: the product's column header compiled for the host)
against the vectors of the compiled reference (tests/golden/cu_bmj_*.npz and cu_bmj_tables.npz, tests/golden/make_golden_bmj.py):
BMJINIT's nine tables and every carried array after every one of the three carried calls, 0 differing bits; the conditions that
keep the fixtures honest; two further seeds against the reference compiled on the spot where its sources are present.  CPU only.

Which cells count for which condition (all of them over the columns of the tile its..ite, jts..jte, after each of the three calls,
from the REFERENCE's vectors):
  deep convection       RAINCV > 0                                                   >= 4 % of the columns, every fixture, every call
  no convection         RAINCV == 0 and tend%th == tend%qv == 0 on every level      >= 20 %, every fixture, every call
  shallow convection    RAINCV == 0 and a non-zero tend%th or tend%qv somewhere      >= 2 % in at least three fixtures (first call)
  CLDEFI at its clips   CLDEFI == EFIMN and CLDEFI == 1 after the last call          both in at least one fixture
and one fixture each with 8 levels, with kts..kte covering 64 levels, with a -0.0 cell in qc, with a fraction set to 0 and with
tendency_fraction = 0.5."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import bmj_oracle as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
FIELDS = B.STATE3 + B.STATE2 + ["accumulated_precipitation"]
REF = os.environ.get("ICAR_REFERENCE", "/root/reference")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def replay(name):
    c = B.make_case(**B.CASES[name])
    A = B.state(c)
    states = []
    for n in range(B.CALLS):
        B.run_oracle(c, A, n)
        states.append({k: A[k].copy() for k in FIELDS})
    return c, states


@pytest.fixture(scope="module")
def replays():
    return {n: replay(n) for n in B.CASES}


def counts(c, z, n):
    """(deep, shallow, none, columns) of the tile after call n (1-based) from the reference's vectors"""
    rain = B.owned(c, z[f"call{n}_raincv"])
    tend = (B.owned(c, z[f"call{n}_tend_th"]) != 0).any(axis=1) | (B.owned(c, z[f"call{n}_tend_qv"]) != 0).any(axis=1)
    deep = rain > 0
    return int(deep.sum()), int((tend & ~deep).sum()), int((~tend & ~deep).sum()), int(rain.size)


def test_tables_equal_reference():
    z = np.load(os.path.join(GOLDEN, "cu_bmj_tables.npz"))
    mine = B.tables()
    for name, shape in B.TABLES:
        assert z[name].shape == shape and B.bitdiff(mine[name], z[name]) == 0, name
        assert np.isfinite(z[name]).all()
    assert np.float32(z["avgefi"]) == np.float32(B.AVGEFI()) == np.float32(0.6) and np.float32(z["efimn"]) == np.float32(B.EFIMN()) == np.float32(0.2)


@pytest.mark.parametrize("name", list(B.CASES))
def test_restatement_equals_reference_vectors(replays, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert json.loads(str(z["params"])) == B.CASES[name]
    c, states = replays[name]
    assert float(z["input_fingerprint"]) == B.fingerprint(c), "the recipe's inputs drifted: rerun tests/golden/make_golden_bmj.py"
    for n in range(B.CALLS):
        s = states[n]
        for k in FIELDS:
            assert sha(s[k]) == str(z[f"sha_call{n + 1}_{k}"]), f"{name}: {k} after call {n + 1} differs from the compiled reference"
            assert np.isfinite(s[k]).all()
        for k in B.STATE2 + ["accumulated_precipitation", "tend_th", "tend_qv"]:
            assert B.bitdiff(s[k], z[f"call{n + 1}_{k}"]) == 0, (name, n + 1, k)
        assert list(z["counts"][n]) == list(counts(c, z, n + 1))
    for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice"):
        assert B.bitdiff(states[-1][k], z[f"call{B.CALLS}_{k}"]) == 0, (name, k)
    # the top level keeps a zero tendency; nothing outside the tile's columns moved but a -0.0 that became +0.0
    assert not states[-1]["tend_qv"][:, -1, :].any() and not states[-1]["tend_th"][:, -1, :].any()
    its, ite, jts, jte = B.tile_of(c)
    out = np.ones(c["water_vapor"].shape, bool); out[jts - 1:jte, :, its - 1:ite] = False
    assert np.array_equal(states[-1]["water_vapor"][out], c["water_vapor"][out])
    assert np.array_equal(states[-1]["potential_temperature"][out], c["potential_temperature"][out])


def test_fixture_conditions():
    shallow_fixtures, clip_lo, clip_hi = 0, False, False
    seen = dict(lev8=False, lev64=False, negzero=False, frac0=False, half=False)
    for name, p in B.CASES.items():
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        c = B.make_case(**p)
        for n in range(1, B.CALLS + 1):
            deep, shallow, none, cols = counts(c, z, n)
            assert deep >= 0.04 * cols, (name, n, deep, cols)
            assert none >= 0.20 * cols, (name, n, none, cols)
        deep, shallow, none, cols = counts(c, z, 1)
        shallow_fixtures += shallow >= 0.02 * cols
        ce = B.owned(c, z[f"call{B.CALLS}_cldefi"])
        clip_lo = clip_lo or bool((ce == np.float32(B.EFIMN())).any())
        clip_hi = clip_hi or bool((ce == np.float32(1.0)).any())
        ny, nz, nx = c["density"].shape
        seen["lev8"] |= nz == 8
        seen["lev64"] |= nz == 64
        fr = c["fractions"]
        seen["frac0"] |= any(f == 0.0 for f in fr)
        seen["half"] |= c["tendency_fraction"] == 0.5 and fr == [0.5] * 4
        if c["negzero"]:
            qc0, qc3 = c["cloud_water"], z[f"call{B.CALLS}_cloud_water"]
            neg = np.signbit(qc0) & (qc0 == 0)
            its, ite, jts, jte = B.tile_of(c)
            assert neg[jts - 1:jte, :, its - 1:ite].any(), "the -0.0 cell lies in the tile"
            assert not np.signbit(qc3[neg]).any() and B.bitdiff(qc3[~neg], qc0[~neg]) == 0, "x + 0: -0.0 becomes +0.0, all else is kept"
            qi0, qi3 = c["cloud_ice"], z[f"call{B.CALLS}_cloud_ice"]
            negi = np.signbit(qi0) & (qi0 == 0)
            assert negi[:, :, 0].any() and not np.signbit(qi3[negi]).any(), "over all i of memory, the halo column included"
            seen["negzero"] = True
        if any(f == 0.0 for f in fr):
            k = ["water_vapor", "cloud_water", "potential_temperature", "cloud_ice"][fr.index(0.0)]
            assert B.bitdiff(z[f"call{B.CALLS}_{k}"], c[k]) == 0 and (z["call1_tend_th"] != 0).any(), "a fraction of 0 leaves the field alone"
    assert shallow_fixtures >= 3, shallow_fixtures
    assert clip_lo and clip_hi
    assert all(seen.values()), seen


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not present")
@pytest.mark.parametrize("seed,nz", [(21, 17), (22, 33)])
def test_further_seeds_against_the_compiled_reference(seed, nz, tmp_path_factory):
    import make_golden_bmj as G
    global _REFLIB
    try:
        L = _REFLIB
    except NameError:
        L = _REFLIB = G.build_reference(str(tmp_path_factory.mktemp("curef")))
    c = B.make_case(nx=22, ny=14, nz=nz, seed=seed, rh_lo=0.5)
    G.ref_init(L, c)
    A, O = B.state(c), B.state(c)
    for n in range(B.CALLS):
        G.ref_call(L, c, A, n)
        B.run_oracle(c, O, n)
        assert not any(G.differing(A, O).values()), (seed, n + 1, G.differing(A, O))
    assert (A["raincv"] > 0).any() and (A["tend_th"] != 0).any()

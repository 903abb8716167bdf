"""The CPU restatement of the forcing update (icar_amd/csrc/forcing_interp.h compiled for the host, tests/forcing_oracle.py) against
the vectors of the compiled reference: the six fixtures of tests/golden/make_golden_forcing.py everywhere, bit for bit, with their
coverage shares; and, where the reference sources are present, the generator's own comparison of all eight cases (six fixtures, two
further seeds) with the reference compiled afresh."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import forcing_oracle as FO

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
REFERENCE = os.path.join(os.environ.get("ICAR_REFERENCE", "/root/reference"), "src")
_results = {}


def result(name):
    if name not in _results:
        c, z = FO.load_case(name)
        _results[name] = (c, z, FO.run_oracle(c, diag=True))
    return _results[name]


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_restatement_reproduces_the_fixture(name):
    import make_golden_forcing as G
    c, z, res = result(name)
    mine = G.flatten(res)
    held = json.loads(str(z["sha"]))
    assert sorted(held) == sorted(mine)
    differing = [k for k in held if FO.sha(mine[k]) != held[k]]
    assert not differing, differing
    full = [k for k in mine if k in z.files]
    assert len(full) >= 4, full
    for k in full:
        assert FO.bitdiff(mine[k], z[k]) == 0, (k, FO.bitdiff(mine[k], z[k]))
        assert np.isfinite(z[k]).all() and float(np.abs(z[k]).max()) > 0, k


@pytest.mark.parametrize("name", sorted(FO.CASES))
def test_coverage_shares_are_the_fixture_s(name):
    import make_golden_forcing as G
    c, z, res = result(name)
    cov = G.coverage(c, res[4])
    held = json.loads(str(z["coverage"]))
    assert cov == held, (cov, held)


def test_every_condition_is_reached_in_some_fixture():
    best = {}
    for name in FO.CASES:
        z = np.load(os.path.join(FO.GOLDEN, name + ".npz"))
        for k, v in json.loads(str(z["coverage"])).items():
            best[k] = max(best.get(k, 0.0), v)
    want = {"vlut_interior", "vlut_below", "vlut_above", "pad_copy", "pad_repeat", "findz_stay1", "findz_jump", "findz_exit", "dz_pos", "dz_neg"}
    assert set(best) == want
    assert all(v >= 0.02 for v in best.values()), best


def test_the_cases_are_what_their_names_say():
    a, b, c_, d, e, f = (FO.CASES[n] for n in sorted(FO.CASES))
    assert a["nzf"] > a["nz"] and b["nzf"] < b["nz"] and c_["nzf"] == c_["nz"] and c_["model_top"] > c_["forcing_top"]
    assert d["shear"] != 0 and d["rot"] != 0 and d["edge"]
    assert e["ext"].count(0) == 2 and e["nsmooth"] == 1
    assert f["nsmooth"] == 3 and f["nx"] == 5 and 2 * f["nsmooth"] + 1 > f["nx"] and f["negzero"]
    cf, _ = FO.load_case(sorted(FO.CASES)[5])
    assert np.signbit(cf["lo1"]["water_vapor"][:, 1, :]).all()


def test_negative_zero_plane_gives_positive_zero():
    """geo_interp starts its sums at 0: a plane of -0.0 in the forcing gives +0.0 wherever only that plane is read"""
    c, z, res = result(sorted(FO.CASES)[5])
    G = c["geo"]
    lo = np.full(c["lo1"]["water_vapor"].shape, -0.0, FO.f32)
    out = FO.geo_vinterp(lo, G)
    assert (out == 0).all() and not np.signbit(out).any()


def test_smoothing_the_same_forcing_array_twice_is_visible():
    c, z, res = result(sorted(FO.CASES)[0])
    lo = c["lo1"]["u"].copy()
    once = FO.interp_wind(lo, c["geo_u"], c["nsmooth"], (c["z"].shape[0], c["z"].shape[1], c["z"].shape[2] + 1))
    twice = FO.interp_wind(lo, c["geo_u"], c["nsmooth"], once.shape)
    assert FO.bitdiff(once, res[0]["u"]) == 0 and FO.bitdiff(once, twice) > 0


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not present on this host")
def test_all_eight_cases_against_the_reference_compiled_afresh():
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_forcing.py"), "--dry"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if "plain differs in" in l]
    assert len(lines) == len(FO.CASES) + len(FO.EXTRA_SEEDS) == 8
    for l in lines:
        assert "plain differs in 0 bits" in l and "| geo_z 0 " in l and "FMA in 0 |" not in l, l

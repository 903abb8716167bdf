"""The CPU restatement of the 2-D forced variables (icar_amd/csrc/forcing2d_cell.h compiled for the host) against the vectors the
compiled reference produced (tests/golden/forcing2d_*.npz, made by tests/golden/make_golden_forcing2d.py): every cell of every array
after every stage, bit for bit.  CPU only.  The arithmetic has no branch, so there are no coverage shares to meet; what the inputs must
contain (zeros, -0.0, a constant field, a dt that is no REAL(4)) is asserted here."""
import os
import subprocess

import numpy as np
import pytest

import forcing2d_oracle as F2

HERE = os.path.dirname(os.path.abspath(__file__))
NSTAGES = 4 * (1 + 2 * 2 + 5) + 5                                 # four variables: init, 2 x (pre, dq), 5 applies; acc after each apply


@pytest.fixture(scope="module")
def cases():
    return {n: F2.load_case(n) for n in F2.CASES}


@pytest.mark.parametrize("name", list(F2.CASES))
def test_restatement_reproduces_the_reference_everywhere(cases, name):
    c, z, _ = cases[name]
    mine = F2.run_oracle(c)
    stored = set(z.files) - {"lut_sha", "input_fingerprint"}
    assert set(mine) == stored and len(mine) == NSTAGES
    bad = {k: F2.bitdiff(mine[k], z[k]) for k in mine if F2.bitdiff(mine[k], z[k])}
    assert not bad, bad
    for k in mine:
        assert mine[k].shape == (c["ny"], c["nx"]) and mine[k].dtype == (np.float64 if k.endswith("_acc") else np.float32)


def test_the_contracted_form_is_another_function(cases, tmp_path):
    import ctypes
    L1 = ctypes.CDLL(F2.build(force=True, contract=True, out=str(tmp_path / "libf2_fma.so")))
    assert L1.f2o_contract() == 1 and F2.lib().f2o_contract() == 0
    c, z, _ = cases["forcing_a_below_37x9x23"]
    fma = F2.run_oracle(c, L=L1)
    assert sum(F2.bitdiff(fma[k], z[k]) for k in fma) > 0


def test_inputs_hold_what_the_cases_are_for(cases):
    assert any(float(np.float32(dt)) != dt for dts in F2.APPLY_DT for dt in dts) and len({dt for dts in F2.APPLY_DT for dt in dts}) >= 3
    for name, (c, z, _) in cases.items():
        for lo in c["lo"]:
            assert 270.0 <= lo["sst"].min() and lo["sst"].max() <= 300.0
            for k in ("shortwave", "longwave"):
                assert 0.0 <= lo[k].min() and lo[k].max() <= 1000.0
            assert (lo["shortwave"] == 0).any() and (lo["external_precipitation"] == 0).mean() >= 0.2
            assert (lo["external_precipitation"] > 0).any()
    lw = [lo["longwave"] for lo in cases[F2.CONSTANT_CASE][0]["lo"]]
    assert all((a == a.flat[0]).all() for a in lw)
    nz = cases[F2.NEGZERO_CASE][0]["lo"][0]
    assert np.signbit(nz["shortwave"][nz["shortwave"] == 0]).all() and np.signbit(nz["external_precipitation"][nz["external_precipitation"] == 0]).all()
    # ... and the interpolation of a field of negative zeros is +0 where every corner is one (the sums start from 0)
    c = cases[F2.NEGZERO_CASE][0]
    out = F2.geo_interp2d(np.full_like(nz["sst"], -0.0), c["G"])
    assert (out == 0).all() and not np.signbit(out).any()


@pytest.fixture(scope="module")
def bounds_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("f2bounds") / "forcing2d_bounds")
    cmd = ["gcc", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "support", "forcing2d_bounds_main.c"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_clean(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("forcing2d_bounds: ")
    return r.stdout


def test_sanitizers_find_nothing_on_the_smallest_grids(bounds_program):
    assert "3 x 3 from 2 x 2" in run_clean([bounds_program])


def test_sanitizers_find_nothing_on_a_fixture_s_tables(bounds_program, cases, tmp_path):
    c, _, _ = cases["forcing_f_wide_5x6x14"]
    G, lo = c["G"], c["lo"][0]["sst"]
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([c["nx"], c["ny"], lo.shape[1], lo.shape[0]], np.int32).tobytes())
        for a in (G["x"].astype(np.int32), G["y"].astype(np.int32), G["w"].astype(np.float32), lo):
            f.write(np.ascontiguousarray(a).tobytes())
    run_clean([bounds_program, src, dst])
    out = np.fromfile(dst, np.float32).reshape(c["ny"], c["nx"])
    assert F2.bitdiff(out, F2.geo_interp2d(lo, G)) == 0

"""What the geometry sweep of tests/test_gpu_step_rows_geometry.py rests on, checked without a GPU:
  * every case of the sweep is finite and has positive jacobians (the 900 m hill of test_gpu_step_rows.py has not, for thin columns);
  * the numpy restatements of tests/step_rows_case.py (written from the Fortran statements) equal the C oracle bit for bit at every
    shape of the sweep, so the device is held to two independent statements of each row;
  * the shape lists reach what they are there for: all four values of n3 % 4, a second trip of the grid-stride loops;
  * every planted extreme moves the strictness-3 Courant maximum and maxval(abs()) of its array: a kernel that skips the planted
    face or cell cannot return the asserted numbers."""
import numpy as np
import pytest
import step_rows_case as S
from util import bits_equal

f32 = np.float32
SHAPES = S.width_shapes() + S.level_shapes()


@pytest.fixture(scope="module")
def big():
    return S.case(*S.BIG, seed=29)


def test_shape_lists_reach_every_edge(big):
    shapes = S.width_shapes()
    assert [s[0] for s in shapes] == S.WIDTHS and shapes[0] == (3, 3, 2), "the smallest tile a context takes comes first"
    assert {s[1] for s in shapes} == {3, 4} and {s[2] for s in shapes} == {2, 3, 4, 5}
    assert {(nx * ny * nz) % 4 for nx, ny, nz in shapes} == {0, 1, 2, 3}, "k_diag_cell's scalar tail: 0, 1, 2 and 3 cells"
    for edge in (64, 256):                                              # a partial, an exactly full and a just-started wave / block
        assert {edge - 1, edge, edge + 1} <= set(S.WIDTHS)
    assert {62, 63} <= {nx - 2 for nx in S.WIDTHS} and {64, 65} <= {nx - 2 for nx in S.WIDTHS}, "k_diag_wreal: waves of nx - 2"
    assert {64, 65} <= {nx + 1 for nx in S.WIDTHS}, "k_wgr_restagger: waves of nx + 1"
    assert {nz % 4 for _, _, nz in S.level_shapes()} == {0, 1, 2, 3} and min(S.LEVELS) == 2 and max(S.LEVELS) > 8
    nx, ny, nz = S.BIG
    assert nx * ny * nz > 2048 * 256 and (nx + 1) * ny * nz > 2048 * 256 and nx * (ny + 1) * nz > 2048 * 256
    assert (nx * ny * nz) % 4 == 1 and big["w"].size == nx * ny * nz
    for at in S.BIG_PLANT_INDICES[1:]:
        assert at in (512 * 256, 2048 * 256) and at < nx * ny * nz - 1


def test_every_case_is_finite_with_positive_jacobians(big):
    for nx, ny, nz in SHAPES + [S.PLANT_SHAPE]:
        c = S.case(nx, ny, nz, seed=nx + nz)                            # (the builder asserts both)
        assert c["u"].shape == (ny, nz, nx + 1) and c["v"].shape == (ny + 1, nz, nx) and np.abs(c["w"]).max() > 0
    S.check_case(big)
    # ... which the same case over the 900 m hill of test_gpu_step_rows.py does not meet at the thin shapes
    from icar_amd import ideal
    with np.errstate(all="ignore"):
        assert float(ideal.make_case(129, 3, 4, hill_height=900.0)["jacobian"].min()) < 0


def restatement_vs_oracle(oracle, c, label):
    dx = float(c["dx"])
    geo = (c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"])
    bad = []

    def same(name, got, want):
        if not bits_equal(got, want):
            bad.append(f"{label} {name}")
    same("max_courant", S.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], dx), f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], dx)))
    w = oracle.balance_uvw(c["u"], c["v"], *geo, dx)
    same("balance_uvw", S.balance_uvw(c["u"], c["v"], *geo, dx), w)
    same("max_courant(balanced w)", S.max_courant(c["u"], c["v"], w, c["dz_levels"], dx), f32(oracle.max_courant(c["u"], c["v"], w, c["dz_levels"], dx)))
    oracle.set_math_mode(0)
    ref = oracle.diagnostic_update(c["pressure"], c["potential_temperature"], c["u"], c["v"], c["w"], c["dzdx"], c["dzdy"], c["jacobian"])
    mine = S.diagnostics(c, ref["exner"])
    assert set(mine) == set(ref) - {"exner"}
    for k, a in mine.items():
        if k == "w_real":
            assert np.isnan(a[0]).all() and np.isnan(a[:, :, 0]).all() and np.isfinite(a[1:-1, :, 1:-1]).all()
            same(k, a[1:-1, :, 1:-1], ref[k][1:-1, :, 1:-1])
        else:
            same(k, a, ref[k])
    rng = np.random.default_rng(5)
    for name in ("water_vapor", "u", "v"):
        x = c[name]
        dq = (1e-3 * rng.standard_normal(x.shape)).astype(np.float32) * f32(np.abs(x).max())
        for fb, flags in ((0, (1, 1, 1, 1)), (1, (1, 1, 1, 1)), (1, (1, 0, 0, 0)), (1, (0, 1, 0, 0)), (1, (0, 0, 1, 0)), (1, (0, 0, 0, 1)), (1, (0, 0, 0, 0))):
            want = x.copy()
            oracle.apply_forcing(want, dq, 37.123456789, fb, *flags)
            got = S.apply_forcing(x, dq, 37.123456789, fb, *flags)
            same(f"apply_forcing {name} fb={fb} {flags}", got, want)
            m = S.forcing_mask(x.shape, *flags) if fb else np.ones(x.shape, bool)
            assert bits_equal(got[~m], x[~m]) and (not m.any() or (got[m] != x[m]).any())
    neg = c["water_vapor"].copy(); neg.reshape(-1)[::3] *= f32(-1)
    want = neg.copy(); oracle.enforce_limits(want)
    same("enforce_limits", S.enforce_limits(neg), want)
    for name in ("u", "v", "w"):
        assert float(S.maxabs(c[name])) == max(float(c[name].max()), -float(c[name].min()))
    return bad


def test_restatements_equal_the_oracle_bit_for_bit(oracle, big):
    bad = []
    for nx, ny, nz in SHAPES:
        bad += restatement_vs_oracle(oracle, S.case(nx, ny, nz, seed=nx + nz), f"{nx}x{ny}x{nz}")
    bad += restatement_vs_oracle(oracle, big, "big")
    assert not bad, bad


def test_planted_extremes_move_every_maximum(oracle, big):
    def cell(c):
        got = f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))
        assert bits_equal(S.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])), got)
        return got
    base, plants = S.planted_cases()
    m0 = cell(base)
    assert len(plants) == 9 and len({label for label, _ in plants}) == 9
    for label, c in plants:
        S.check_case(c)
        name = label[0]
        m = cell(c)
        print(f"{label}: strictness-3 maximum {m} (unplanted {m0})")
        assert m > m0 and m >= 100.0, label
        assert S.maxabs(c[name]) == -S.PLANT and S.maxabs(base[name]) < 100.0, label
        assert sum(int((c[k] != base[k]).sum()) for k in ("u", "v", "w")) == 1, label
    m0 = cell(big)
    for label, c in S.big_planted_cases(big):
        assert cell(c) > m0, label
        for name in ("u", "v", "w"):
            assert S.maxabs(c[name]) == -S.PLANT and int((c[name] != big[name]).sum()) == 1, (label, name)

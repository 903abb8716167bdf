"""What the geometry sweep of tests/test_gpu_wind_rows_geometry.py rests on, checked without a GPU:
  * the shape lists of tests/wind_rows_case.py reach what they are there for: nx and nx + 1 on both sides of 64, every nz % 4, the
    second block of 64 levels, ny on both sides of the smoothing window, n3 on and off a multiple of 256, odd, even and prime
    transform lengths;
  * the numpy restatement of spatial_winds (written from the Fortran statements) equals the C oracle bit for bit at every case of
    the sweep after both passes, so the device is held to two independent statements of row W2;
  * the planted case and its two option sets take every arm of calc_direction, calc_weight and the two N^2 clamps -- counted from
    the restatement's bracket state, a condition of the test and not a measurement;
  * fftshift / ifftshift invert each other at the odd transform sizes, and the look-up tables built there are finite and not small."""
import numpy as np
import pytest
import wind_rows_case as S
from icar_amd.grid import grid_t
from oracle import wind_oracle as W
from util import bits_equal, nbitdiff
from wind_case import terrain, lut_options

f32 = np.float32


def test_shape_lists_reach_every_edge():
    for cases, reason in ((S.width_cases(), "widths"), (S.level_cases(), "levels")):
        assert all(c["smooth_nsq"] for c in cases), reason
    widths = S.width_cases()
    assert [c["nx"] for c in widths] == S.WIDTHS and widths[0]["nx"] == S.WIDTH_WINSZ + 1
    for edge in (64, 128):
        assert {edge - 1, edge, edge + 1} <= set(S.WIDTHS) and {edge, edge + 1} <= {nx + 1 for nx in S.WIDTHS}
    assert 63 in {nx + 1 for nx in S.WIDTHS}
    assert {c["ny"] for c in widths} == {3, 4} and {c["nz"] for c in widths} == {2, 3, 4, 5}
    assert all(c["nx"] > c["winsz"] for c in S.sweep_cases() if c["smooth_nsq"]), "the device refuses nx <= winsz with smooth_nsq"
    levels = S.level_cases()
    assert [(c["nx"], c["ny"]) for c in levels] == [(6, 3)] * len(S.LEVELS)
    assert {c["nz"] % 4 for c in levels} == {0, 1, 2, 3} and min(S.LEVELS) == 2 and {63, 64, 65} <= set(S.LEVELS)
    rows = S.row_cases()
    w = S.ROW_WINSZ
    assert [c["ny"] for c in rows] == [w - 1, w, w + 1, 2 * w + 1, 2 * w + 2] and all(c["winsz"] == w and c["smooth_nsq"] for c in rows)
    for c in S.window_cases():
        assert (c["nx"], c["ny"], c["nz"]) == (9, 5, 4) and c["nx"] > c["winsz"] and c["smooth_nsq"] and c["variable_N"]
    assert {c["vsmooth"] - 4 for c in S.window_cases()} >= {-1, 0, 3} and any(c["winsz"] >= 4 for c in S.window_cases())
    sweep = S.sweep_cases()
    n3 = {(c["nx"] * c["ny"] * c["nz"]) % 256 == 0 for c in sweep}
    assert n3 == {True, False}, "k_lw_exp: blocks of 256 over n3, full and partial last block"
    assert len({c["label"] for c in sweep}) == len(sweep) and 24 <= len(sweep) <= 48, "a few dozen small cases"
    # the option sets all occur, and not only at one shape list
    assert {(c["variable_N"], c["smooth_nsq"]) for c in sweep} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c["hydrometeors"] for c in sweep} == set(S.HYDROMETEORS) and {c["update"] for c in sweep} == {True, False}
    assert {c["axes"] for c in sweep} == set(S.AXES) and S.AXES[1] == (2, 2, 2) and S.PASSES == 2
    for cases in (widths, levels, rows, S.window_cases()):
        assert {c["update"] for c in cases} == {True, False} and len({c["hydrometeors"] for c in cases}) >= 2 and len({c["axes"] for c in cases}) == 2
    # smooth_array's running row sums: w > nrow, w == nrow, w < nrow (array_utilities.f90:363-368)
    smoothed = [c for c in sweep if c["smooth_nsq"]]
    assert any(c["winsz"] > c["ny"] for c in smoothed) and any(c["winsz"] == c["ny"] for c in smoothed) and any(c["winsz"] < c["ny"] for c in smoothed)
    # vertical windows cut off at the top, at the bottom and at both ends.  The one of the stability / vertical smoothing looks up
    # only, and down by what the top cut off: it cannot be cut at the bottom alone ...
    clips = set().union(*(S.window_clips(c["nz"], c["vsmooth"], True) for c in sweep if c["variable_N"] and c["smooth_nsq"]))
    assert clips == {"none", "top", "both"}, clips
    # ... the j -+ winsz one of the N^2 mean can
    clips = set().union(*(S.window_clips(c["nz"], c["winsz"], False) for c in sweep))
    assert clips == {"none", "top", "bottom", "both"}, clips
    # W3: odd x even, even x odd, odd x odd, a prime length, and nx + 1 on 64 / 65
    sizes = [S.transform_size(*s) for s in S.W3_SIZES]
    assert sizes == [(43, 38), (42, 39), (43, 39), (73, 31), (74, 30)]
    parity = {(a % 2, b % 2) for a, b in sizes}
    assert {(1, 0), (0, 1), (1, 1)} <= parity and all(43 % p for p in range(2, 7))
    assert [s[0] + 1 for s in S.W3_SIZES[3:]] == [64, 65]
    assert S.transform_size(*S.TILED) == (43, 39) and S.transform_size(*S.VARYING) == (43, 38)
    for s in S.W3_SIZES[3:]:                          # k_lut_transpose: slab * ncombo on a multiple of 256 for one table, off it for the other
        nd, ns, nn = S.W3_AXES
        assert {((s[0] + 1) * len(S.DZ_LEVELS) * nd * ns * nn) % 256 == 0, (s[0] * len(S.DZ_LEVELS) * nd * ns * nn) % 256 == 0} == {True, False}
    zb, zt = S.layer_bounds()
    assert [W.n_steps_of(b, t, S.MINIMUM_LAYER_SIZE) for b, t in zip(zb, zt)] == [1, 1, 2, 4]
    # the tilings: 2 x 2 and 3 x 2 images, neighbours share two cells, every image has an offset but the first
    for nimages, split in zip(S.TILINGS, ((2, 2), (3, 2))):
        gs = [grid_t().set_grid_dimensions(S.TILED[0], S.TILED[1], 4, nimages, im) for im in range(1, nimages + 1)]
        assert (gs[0].ximages, gs[0].yimages) == split
        assert gs[0].ime - gs[1].ims + 1 == 2 and sum(g.ims > 1 or g.jms > 1 for g in gs) == nimages - 1
    t = terrain(S.VARYING[0], S.VARYING[1], seed=6)
    sub = S.varying_sublayers(*S.varying_layers(t))
    assert len(set(sub)) > 1 and min(sub) >= 1, f"space_varying_dz: nsub < maxsub must occur, sub-layers per level {sub}"


def compare(oracle, c, states=None):
    x = S.inputs(c)
    oracle.set_math_mode(0)
    want = S.run(oracle.spatial_winds, c, x)
    got = S.run(S.spatial_winds, c, x, states=states)
    bad = []
    for n, g, w in zip(S.FIELDS, got, want):
        assert np.isfinite(g).all() and np.isfinite(w).all(), f"{c['label']} {n}: not finite"
        if not bits_equal(g, w):
            at = np.argwhere(g.view(np.int32) != w.view(np.int32))[0]
            bad.append(f"{c['label']} {n}: {nbitdiff(g, w)} of {g.size} differ, first at (j, k, i) = {tuple(int(a) for a in at)}")
    assert abs(got[2]).max() > 0.1 and abs(got[3]).max() > 0.1, f"{c['label']}: the perturbation is trivial"
    assert not bits_equal(got[0], x["a"]["u"]) and got[4].min() > 0
    return bad


def test_restatement_equals_the_oracle_bit_for_bit(oracle):
    bad = []
    for c in S.sweep_cases():
        bad += compare(oracle, c)
    assert not bad, bad


def test_planted_case_takes_every_branch(oracle):
    states = {}
    for second in (False, True):
        c = S.planted_case(second)
        states[second] = []
        bad = compare(oracle, c, states[second])
        assert not bad, bad
    nx, ny, nz = S.PLANT_SHAPE
    first = states[False][0]                          # the first pass of the first option set: the planted winds are still exact
    # calc_direction returns what the reference's statements give for the planted pairs
    want = {(0.0, 0.0): 4.712389, (5.0, 0.0): 1.5707964, (-5.0, 0.0): 4.712389, (0.0, 4.0): 0.0, (0.0, -4.0): 3.1415927,
            (-1e-6, 6.0): 6.2831855, (6.0, 8.0): None, (40.0, 20.0): None}
    for r in S.PLANT_ROWS:
        for n, face in enumerate(S.PLANT_FACES):
            pu, pv = S.PLANTS[(n + 3 * r) % len(S.PLANTS)]
            assert first["curspd"][r, face] == f32(np.sqrt(f32(pu) * f32(pu) + f32(pv) * f32(pv))), (r, face)
            if want[(pu, pv)] is not None:
                assert first["curdir"][r, face] == f32(want[(pu, pv)]), (r, face, pu, pv, first["curdir"][r, face])
    x = S.inputs(S.planted_case())
    nd, ns, nn = len(x["dirv"]), len(x["spdv"]), len(x["nsqv"])
    assert x["dirv"][2] == first["curdir"][0, 1] and x["spdv"][1] == f32(10) and x["dirv"][-1] == f32(6.2831855)
    every = [s for second in (False, True) for s in states[second]]
    arms = set().union(*(set(np.unique(s["arm"]).tolist()) for s in every))
    assert arms == set(range(len(S.ARMS))), f"calc_direction arms taken: {[S.ARMS[a] for a in sorted(arms)]}"

    def reached(cond):
        return any(bool(cond(s).any()) for s in every)
    # bestpos == n on each axis (next == n, weight 1): the speed axis with the first set already, the other two with the second
    assert (first["spos"] == ns).any() and (first["nexts"][first["spos"] == ns] == ns).all()
    assert reached(lambda s: s["dpos"] == nd) and reached(lambda s: s["npos"] == nn)
    # match < d(1) on each axis (next == 1, weight 1)
    x2 = S.inputs(S.planted_case(True))
    for s in states[True]:
        for name, axis, nxt, wgt in (("curdir", x2["dirv"], "nextd", "dweight"), ("curspd", x2["spdv"], "nexts", "sweight"),
                                     ("curnsq", x2["nsqv"], "nextn", "nweight")):
            low = s[name] < axis[0]
            assert low.any(), f"match < d(1) not reached on {name}"
            assert (s[nxt][low] == 1).all() and (s[wgt][low] == 1).all()
    # a weight of exactly 0 (a value on an axis point: direction 2 pi on dirmax, speed 10 on spdv(2)) and of exactly 1
    assert (first["dweight"] == 0).any() and (first["sweight"] == 0).any()
    assert reached(lambda s: s["dweight"] == 1) and reached(lambda s: s["sweight"] == 1) and reached(lambda s: s["nweight"] == 1)
    # both clamps of N^2
    assert first["at_min"].sum() > 0 and first["at_max"].sum() > 0
    print(f"planted case: {int(first['at_min'].sum())} cells on min_stability, {int(first['at_max'].sum())} on max_stability")
    assert first["at_min"][:, :, S.UNSTABLE_COLUMNS].any() and first["at_max"][:, :, S.INVERSION_COLUMNS].any()


@pytest.mark.parametrize("size", S.W3_SIZES + [S.TILED])
def test_odd_transform_sizes_on_the_cpu(size):
    nxg, nyg, buffer = size
    fx, fy = S.transform_size(*size)
    rng = np.random.default_rng(fx * fy)
    x = (rng.standard_normal((fx, fy)).astype(np.float32) + 1j * rng.standard_normal((fx, fy)).astype(np.float32)).astype(np.complex128)
    assert np.array_equal(W.ifftshift2cc(W.fftshift2cc(x)), x)
    if fx % 2:
        assert not np.array_equal(W.fftshift2cc(W.fftshift2cc(x)), x), "odd n: fftshift is not its own inverse"
    lt_o = S.w3_options(buffer)
    tf, lt, buf = W.setup_linwinds(terrain(nxg, nyg, seed=4).T.copy(), S.W3_DX, buffer)
    assert tf.shape == (fx, fy) and buf == buffer + 2
    zb, zt = S.layer_bounds()
    ul, vl, *_ = W.build_lut(tf, lt, buf, zb, zt, lut_options(lt_o))
    nd, ns, nn = S.W3_AXES
    assert ul.shape == (ns, nd, nn, nxg + 1, len(zb), nyg) and vl.shape == (ns, nd, nn, nxg, len(zb), nyg + 1)
    for a in (ul, vl):
        assert np.isfinite(a).all() and abs(a).max() > 0.05

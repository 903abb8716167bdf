"""What the horizontal sweeps of tests/test_gpu_mpdata_rows.py rest on, checked without a GPU:
  * the launch layout of the fused MPDATA kernel, read from the product's own header (mpdata_geometry.h, through
    tests/support/mpdata_probe.hip), held to the rows written down from the formula before it moved into that header;
  * the shape lists reach every class of layout they are there for: full tiles, one-column tiles, short last chunks, every march
    of a chunk the formula can produce, work-item counts below and beside the 8 XCDs, level ranges with a one-row chunk;
  * every case meets the conditions on its fields, and the oracle's answer is well conditioned at the sweeps' shapes: one ulp on
    every input moves no cell by more than a third of what the device is allowed."""
import numpy as np
import pytest
from icar_amd import ideal
from icar_amd.constants import kADV_MPDATA
import mpdata_rows_case as R
from util import MPDATA_RTOL, MPDATA_MARGIN, adv_args, local_rel_err

# nx, ny, nz, nv -> ntile, nchunk, clen, rows of the last chunk
LAYOUT_PINS = [((512, 512, 40, 9), (9, 3, 170, 170)), ((512, 512, 40, 3), (9, 9, 57, 54)), ((1024, 1024, 40, 3), (18, 14, 73, 73)),
               ((258, 130, 40, 9), (5, 5, 26, 24)), ((256, 256, 40, 9), (5, 11, 24, 14)), ((256, 128, 80, 3), (5, 5, 26, 22)),
               ((100, 100, 30, 3), (2, 6, 17, 13)), ((61, 70, 41, 3), (2, 4, 17, 17)), ((70, 10, 9, 3), (2, 1, 8, 8)),
               ((5, 275, 8, 3), (1, 17, 17, 1))]
# nz at nx = 5, ny = 40, nv = 3 -> nkr, kstore, kb, nw, exact
LEVEL_PINS = [(80, (3, 27, 4, 8, False)), (8, (1, 8, 1, 8, True))]


def test_layout_is_the_one_written_down(probe):
    for (nx, ny, nz, nv), want in LAYOUT_PINS:
        g = R.geometry(probe, nx, ny, nz, nv)
        assert (g["ntile"], g["nchunk"], g["clen"], g["last_rows"]) == want, ((nx, ny, nz, nv), g)
        assert sum(c["rows"] for c in g["chunks"]) == ny - 2 and g["chunks"][0]["ja"] == 1 and g["chunks"][-1]["north"]
        assert all(a["jb"] + 1 == b["ja"] for a, b in zip(g["chunks"], g["chunks"][1:]))
    for nz, want in LEVEL_PINS:
        g = R.geometry(probe, 5, 40, nz, 3)
        assert (g["nkr"], g["kstore"], g["kb"], g["nw"], g["exact"]) == want, (nz, g)
    # the two templates of the width and row sweeps
    g9, g8 = R.geometry(probe, 61, 6, 9), R.geometry(probe, 61, 6, 8)
    assert (g9["kb"], g9["nw"], g9["exact"]) == (2, 5, False) and (g8["kb"], g8["nw"], g8["exact"]) == (1, 8, True)
    assert R.geometry(probe, R.XOUT + 2, 6, 9)["ntile"] == 1 and R.geometry(probe, R.XOUT + 3, 6, 9)["ntile"] == 2
    import ctypes
    out = (ctypes.c_int * 64)()
    assert probe.icar_probe_mpdata_geometry(5, 9, 6, 3, out) == 0
    for bad in ((2, 9, 6, 3), (5, 9, 2, 3), (5, 0, 6, 3), (5, 9, 6, 0)):                  # (nx, nz, ny, nv)
        assert probe.icar_probe_mpdata_geometry(*bad, out) != 0


def test_march_schedule_is_a_march(probe):
    """every chunk of every list shape: 4 warm-up steps, steady pairs, a tail; together the steps P0 .. jb + 1, each once; a steady
    step reads rows P-1 .. P+3 without clamping"""
    for name, shapes in R.lists(probe).items():
        for s in shapes:
            nx, ny, nz = s[:3]
            for c in R.geometry(probe, nx, ny, nz, R.shape_nv(s))["chunks"]:
                assert c["P0"] == c["ja"] - 3 and c["s0"] - c["P0"] == 4 and c["npair"] >= 0 and c["ntail"] >= (0 if c["npair"] else 1), (s, c)
                assert 4 + 2 * c["npair"] + c["ntail"] == c["jb"] + 2 - c["P0"], (s, c)
                if c["npair"]:
                    assert c["s0"] - 1 >= 0 and c["s0"] + 2 * c["npair"] - 1 + 3 <= ny - 1, (s, c)


def layouts(probe, shapes):
    return [(s, R.geometry(probe, s[0], s[1], s[2], R.shape_nv(s))) for s in shapes]


def test_lists_reach_their_classes(probe):
    L = R.lists(probe)
    for name, shapes in L.items():
        assert len(set((s[0], s[1], s[2], tuple(s[3])) for s in shapes)) == len(shapes), f"{name}: a shape twice"
    W, RO, S, RA = (layouts(probe, L[k]) for k in ("widths", "rows", "scalars", "ranges"))
    # x tiles: exactly full ones, a last tile of one column, the smallest tile; both templates
    for nz, exact in ((9, False), (8, True)):
        nxs = {s[0]: g for s, g in W if s[2] == nz}
        assert all(g["exact"] == exact for g in nxs.values())
        for t in (1, 2) + ((3,) if nz == 9 else ()):
            full = t * R.XOUT + 2
            assert nxs[full]["ntile"] == t and nxs[full + 1]["ntile"] == t + 1 and full - 1 in nxs, (nz, t)
        assert 3 in nxs and nxs[3]["ntile"] == 1
        assert {63, 64, 65, 126, 127, 128} <= set(nxs)                      # the seams of the exact mode's 63-cell tiles
    assert set(range(3, 131)) | set(range(174, 179)) == {s[0] for s, g in W if s[2] == 9}
    assert all(g["nchunk"] == 1 and g["last_rows"] == 4 for s, g in W)
    # y chunks
    for nx in R.ROW_WIDTHS:
        mine = [(s, g) for s, g in RO if s[0] == nx and s[2] == 9 and s[3] == R.NAMES]
        assert set(range(3, 71)) <= {s[1] for s, g in mine}
        assert {g["last_rows"] for s, g in mine if g["nchunk"] > 1} >= {1, 2, 3, 4, 5, 6}, nx
        assert {2, 3} <= {g["nchunk"] for s, g in mine} and max(g["nchunk"] for s, g in mine) >= 8, nx
        assert {g["ntile"] for s, g in mine} == {1 if nx == 5 else 2}
    assert (61 - 2) - R.XOUT == 1                                            # the second tile of the wider one owns one column
    # the march of a chunk: every (pairs, tail, north ring) the formula produces up to NY_MAX rows is in the lists
    every = R.march_classes(probe)
    hit = R.classes_of(probe, [s for k in L for s in L[k]])
    assert set(every) <= hit, f"march classes no list reaches: {sorted(set(every) - hit)}"
    for pairs in (0, 1, 2):
        assert {k[1] for k in every if k[0] == pairs}, pairs
    assert {k[2] for k in hit} == {True, False}
    print("march classes (pairs, tail steps, touches the north ring):", sorted(every))
    # work items against the 8 XCDs
    n = [g["nitem"] for s, g in S]
    assert 1 in n and any(1 < x < 8 for x in n) and any(x > 8 and x % 8 for x in n) and any(x % 8 == 0 for x in n), n
    assert {R.shape_nv(s) for s, g in S if g["nitem"] == R.shape_nv(s)} == set(range(1, 12))
    assert {R.shape_nv(s) for s, g in S if g["ntile"] == 2 and g["nchunk"] >= 2} == set(range(1, 12))
    # level ranges with a one-row and a two-row last chunk
    assert {(g["nkr"], g["last_rows"]) for s, g in RO + RA if g["nchunk"] > 1 and g["last_rows"] <= 2} >= {(k, r) for k in (1, 2, 3) for r in (1, 2)}
    assert all(g["ntile"] == 2 for s, g in RA) and {g["nkr"] for s, g in RA} == {2, 3}


def test_a_list_without_its_one_row_chunk_is_noticed(probe, monkeypatch):
    """the coverage assertions are not vacuous: without the row counts whose last chunk has one row they fail"""
    L = dict(R.lists(probe))
    L["rows"] = [s for s in L["rows"] if not (lambda g: g["nchunk"] > 1 and g["last_rows"] == 1)(R.geometry(probe, s[0], s[1], s[2], R.shape_nv(s)))]
    assert len(L["rows"]) < len(R.lists(probe)["rows"])
    monkeypatch.setattr(R, "_LISTS", L)
    with pytest.raises(AssertionError):
        test_lists_reach_their_classes(probe)


def all_shapes(probe):
    return [s for k, v in R.lists(probe).items() for s in v]


def test_every_case_meets_its_conditions(oracle, probe):
    for s in all_shapes(probe):
        c = R.rows_case(oracle, *s)
        try:
            R.check_case(c, s[3])
            assert ideal.cfl_dt(c) > 0
        except AssertionError as e:
            raise AssertionError(f"{s[:3]}: {e}")


def conditioning_shapes(probe):
    """the extremes of every list and every eighth shape between them"""
    out = []
    for k, v in R.lists(probe).items():
        out += [v[t] for t in sorted(set(range(0, len(v), 8)) | {0, len(v) - 1})]
    return out


def test_reference_is_well_conditioned_at_the_sweeps_shapes(oracle, probe):
    """Every cell of every input one float ulp up: the oracle's MPDATA (order 2, limiter) moves by at most 1e-6 of the local field
    scale -- a third of the 3e-6 the device is held to (MPDATA_MARGIN x MPDATA_RTOL), so a device that misses at one of these shapes
    misses by its own doing, not because the limiter's thresholds next to the ring sit on a rounding boundary of the inputs."""
    shapes = conditioning_shapes(probe)
    assert len(shapes) >= 20
    bound = 1e-6
    assert 3 * bound <= MPDATA_MARGIN * MPDATA_RTOL * (1 + 1e-9)
    worst, bad = 0.0, {}
    for s in shapes:
        nx, ny, nz, names = s
        c = R.rows_case(oracle, nx, ny, nz, names)
        dt = ideal.cfl_dt(c)
        res = []
        for case in (c, R.nudged(c, names)):
            q = np.stack([case[n] for n in names]).copy()
            oracle.advect(kADV_MPDATA, q, *adv_args(case), dt)
            res.append(q)
        for m, n in enumerate(names):
            err, where = local_rel_err(res[1][m], res[0][m])
            worst = max(worst, err)
            if err > bound:
                bad[(nx, ny, nz, n)] = (err, where)
    print(f"largest response to one ulp on every input over {len(shapes)} shapes: {worst:.3e} of the local field scale")
    assert not bad, bad

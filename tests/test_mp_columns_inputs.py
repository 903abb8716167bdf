"""What the column-height sweeps of tests/test_gpu_mp_columns.py rest on, checked without a GPU:
  * the launch table of Thompson over 1 .. 1024 levels, read from the product's own header (column_comm.h:
    thompson_launch_geometry(), through tests/support/th_probe.hip), and that the sweep's heights reach every row of it;
  * at every height, what the inputs and the oracle alone must meet before a device is compared with them
    (mp_columns_case.check_thompson_oracle / check_simple_oracle): all four species present, rain at the surface, fall speeds carried
    down over several levels and across level 63 / 64, sub-step counts that differ between the columns of one block."""
import numpy as np
import mp_columns_case as M

L, P = M.LANE, M.PACK
# (first nk, last nk, (kind, threads per block, columns per block)) above 36 levels; below, 256-thread blocks of 256 // nk columns
TABLE_ABOVE_36 = [(37, 37, (P, 1024, 27)), (38, 42, (P, 256, 6)), (43, 44, (P, 1024, 23)), (45, 51, (P, 256, 5)), (52, 56, (P, 512, 9)),
                  (57, 64, (L, 256, 0)), (65, 73, (P, 512, 7)), (74, 85, (P, 256, 3)), (86, 102, (P, 512, 5)), (103, 113, (P, 1024, 9)),
                  (114, 128, (P, 256, 2)), (129, 146, (P, 1024, 7)), (147, 170, (P, 512, 3)), (171, 204, (P, 1024, 5)),
                  (205, 256, (P, 256, 1)), (257, 341, (P, 1024, 3)), (342, 512, (P, 512, 1)), (513, 1024, (P, 1024, 1))]


def test_launch_table_and_what_the_sweep_covers(probe):
    """The table as runs of equal launches, held to the one written down when the sweep was designed; 1025 levels are refused; the
    sweep's heights hold a height of every (kind, block size, columns per block) that occurs up to 1024 levels, both sides of every
    boundary of the table up to 130 levels, both sides of 64 / 65 (level masks / flag words), and every height from 2 to 130."""
    table = M.launch_table(probe)
    for a, b, (kind, nt, cpb) in table:
        print(f"nk {a:4d} .. {b:4d}: {M.KIND[kind]:4s} {nt:4d} threads, {cpb:3d} columns per block, in the sweep: {[h for h in M.HEIGHTS if a <= h <= b][:4]} ...")
    assert table[0] == (1, 1, (L, 256, 0))
    low = [r for r in table if 2 <= r[0] <= 36]
    assert all(kind == P and nt == 256 and cpb == 256 // a == 256 // b for a, b, (kind, nt, cpb) in low) and low[0][0] == 2 and low[-1][1] == 36
    assert [r for r in table if r[0] > 36] == TABLE_ABOVE_36
    assert M.launch_geometry(probe, M.TOO_TALL) == (0, 0, 0, 0, 0) and M.launch_geometry(probe, 0)[0] == 0
    heights = set(M.HEIGHTS)
    assert set(range(1, 131)) <= heights and 64 in heights and 65 in heights and not [h for h in range(1, 131) if h not in heights]
    for a, b, g in table:
        assert heights & set(range(a, b + 1)), f"no height of the sweep launches {g}"
        if a <= 130:
            assert a in heights and (a == 1 or a - 1 in heights), f"boundary {a - 1} / {a}"
        assert a in heights and b in heights, f"row {a} .. {b}: the sweep takes both of its ends"
    # BlockComm switches from level masks to flag words behind `nz <= 64`, but Thompson's packed kernel -- the only caller of those
    # exchanges -- never gets 57 .. 64 levels: the heights next to that switch that reach it are 56 and 65, both in the sweep
    assert all(M.launch_geometry(probe, nk)[0] == L for nk in range(57, 65)) and M.launch_geometry(probe, 56)[0] == P == M.launch_geometry(probe, 65)[0]
    # mp_simple takes block_comm_geometry() as it comes: the same blocks as Thompson's packed kernel, and 4 / 256 columns where
    # Thompson runs the lane kernel
    for nk in M.HEIGHTS:
        kind, nt, cpb, snt, scpb = M.launch_geometry(probe, nk)
        assert (snt, scpb) == ((nt, cpb) if kind == P else (256, 256 // nk)), nk


def test_tiles_of_the_sweep_have_partial_and_full_blocks(probe):
    for nk in M.HEIGHTS:
        kind, nt, cpb, snt, scpb = M.launch_geometry(probe, nk)
        for k_, g in ((kind, cpb if kind == P else 4), (P, scpb)):
            nx, ny = M.tile_shape(g)
            sizes = [len(x) for x in M.column_groups(k_, g, nx)]
            assert ny - 2 >= 3 and sizes.count(g) >= 2, (nk, sizes)
            if g > 1:
                assert (sizes[0] < g or k_ == L) and sizes[-1] < g, (nk, sizes)        # (the lane kernel's blocks start at the tile's edge)


def test_thompson_inputs_meet_their_conditions_at_every_height(th_oracle, probe):
    bad = {}
    for nk in M.HEIGHTS:
        kind, nt, cpb = M.launch_geometry(probe, nk)[:3]
        c = M.thompson_case(probe, nk)
        assert float(c["dz_mass"].sum(axis=1).max()) < 1.45 * M.DEPTH and float(c["dz_mass"].sum(axis=1).min()) > 0.5 * M.DEPTH
        assert len(np.unique(c["dz_levels"])) == min(c["nz"], 5)
        ref, plans = M.thompson_oracle_run(th_oracle, c, M.thompson_dt(nk), levels=M.SINGLE_LEVEL if nk == 1 else None)
        try:
            M.check_thompson_oracle(c, ref, plans, kind, cpb)
        except AssertionError as e:
            bad[nk] = str(e)
    assert not bad, bad


def test_mp_simple_inputs_meet_their_conditions_at_every_height(oracle, probe):
    bad = {}
    assert M.SIMPLE_HEIGHTS == M.HEIGHTS[1:]
    for nk in M.SIMPLE_HEIGHTS:
        cpb = M.launch_geometry(probe, nk)[4]
        c = M.simple_case(probe, nk)
        dt = M.simple_dt(nk)
        try:
            M.check_simple_oracle(c, M.simple_oracle_run(oracle, c, dt), dt, cpb)
        except AssertionError as e:
            bad[nk] = str(e)
    assert not bad, bad


def test_layered_case_of_the_80_level_tile(th_oracle):
    """the inputs of test_gpu_mp_columns.py::test_thompson_config4_80_levels_tile_layered on a strip of that tile"""
    c = M.make_case(80, 256, 5)
    ref, plans = M.thompson_oracle_run(th_oracle, c, M.thompson_dt(80), calls=2)
    M.check_thompson_oracle(c, ref, plans, M.PACK, 3)

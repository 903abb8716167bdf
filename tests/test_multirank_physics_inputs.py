"""What tests/test_gpu_multirank_physics.py rests on, checked without a GPU from the restatements alone (tiled_step_case.TileChain on the
host tiles of every decomposition, exchanging through LocalExchange):
  * the owned ranges of the images partition the interior 2..nx-1 x 2..ny-1 for worlds 2, 4 and 8 and halo widths 1 and 2;
  * every tile of every decomposition has land and water columns (both masks: the basic one and Noah's);
  * over the run every tile has convecting columns with BMJ, Tiedtke (ktype /= 0) and NSAS (deep or shallow);
  * lsm's gate opens, stays shut and opens again; the images' own CFL steps differ and lie under the 120 s cap, so co_min decides dt;
  * pbl_simple: at least one tile row's nsubsteps differs from the whole-domain row's, and the tiled chain differs from the one-image
    chain in owned cells of potential_temperature; NSAS: at least one tile row's kbmax / kbm / kmax differs from the whole-domain row's,
    and the tiled chain differs likewise -- a device that took whole-domain bounds would fail the GPU tests;
  * the configurations marked star (no row-coupled scheme, upwind): the tiled chain equals the one-image chain in every owned cell.

Tiedtke's leveltop.  The issue lists it as the third row coupling.  It cannot change a result, on this case or another, and the assertion
made for it here is therefore the opposite one (a Tiedtke run without pbl_simple: tiled == one image), next to the one on the row as the
GPU test runs it (with pbl_simple: tiled /= one image).  The reason, from icar_amd/csrc/tiedtke_column.h (module_cu_tiedtke.f90:2016-2106):
leveltop = min(n - 15, the level whose interface pressure lies within 50 hPa of 250 hPa in the row's first column) only bars mid-level
convection from starting ABOVE it (jk > leveltop, CUBASMC); an updraft that starts in a column without deep or shallow convection is kept
only while jk >= kctop0, the first level above 400 hPa.  A start the two values of leveltop treat differently lies above 300 hPa, hence
above kctop0, and is dropped at once in both.  With 12 levels n - 15 is negative besides.  Tried before this was seen: 24 levels up to
13 km with the hill under the first column (leveltop 5 on five rows of the whole domain, 4 on every tile row of the eastern tiles) and a
saturated, warmed layer at each of the levels 18 .. 21 in 40 % of the columns -- 0 cells of any field differed."""
import copy

import numpy as np
import pytest

import tiled_step_case as TS

WORLDS = (2, 4, 8)


@pytest.fixture(scope="module")
def tab():
    import noah_oracle as N
    return N.load_tables()


@pytest.fixture(scope="module")
def runs(th_oracle, tab):
    """{(configuration, world): chains after the two step() calls}; world 1 is the one-image run.  Made on demand, kept for the module."""
    th_oracle.set_math_mode(0)
    cache, cases = {}, {}

    def get(name, world, cfg=None):
        if (name, world) not in cache:
            cfg = cfg or TS.CONFIGS[name]
            if name not in cases:
                c, dq, nc = TS.whole_case(th_oracle, cfg, tab)
                cases[name] = (c, dq, nc) + TS.schedule(th_oracle, c)
            c, dq, nc, ui, ends = cases[name]
            chains = TS.chains_of(th_oracle, cfg, world, c, dq, nc, tab, ui)
            counts, clocks = TS.run(chains, ends, TS.LocalExchange(chains))
            assert all(np.isfinite(a).all() for ch in chains for a in ch.s.values()), (name, world)
            cache[name, world] = (chains, counts, clocks)
        return cache[name, world]
    return get


def differing(chains, one, field="potential_temperature"):
    """the number of owned cells in which the tiled chains differ from the one-image chain"""
    n = 0
    for ch in chains:
        lo, gl = TS.owned(ch.g)
        a = ch.acc if field == "acc" else ch.s[field]
        b = one.acc if field == "acc" else one.s[field]
        n += TS.nbits(TS.own(a, lo), TS.own(b, gl))
    return n


def test_owned_ranges_partition_the_interior():
    for world in WORLDS:
        for halo in (1, 2):
            owned = np.zeros((TS.NYG, TS.NXG), np.int32)
            for image in range(1, world + 1):
                g = TS.grid_of(world, image, halo)
                owned[g.jts - 1:g.jte, g.its - 1:g.ite] += 1
                assert g.ims >= 1 and g.ime <= TS.NXG and g.jms >= 1 and g.jme <= TS.NYG
                its, ite, jts, jte = TS.local_bounds(g)
                assert its - 1 == (1 if g.west_boundary else halo) and g.ime - g.ite == (1 if g.east_boundary else halo)
                assert jts - 1 == (1 if g.south_boundary else halo) and g.jme - g.jte == (1 if g.north_boundary else halo)
            assert (owned[1:-1, 1:-1] == 1).all() and owned[0].sum() == 0 and owned[-1].sum() == 0 and owned[:, 0].sum() == 0 and owned[:, -1].sum() == 0, (world, halo)
    # the decompositions the GPU tests run: a seam on one side only, 2 x 2, and 4 x 2 with seams on three sides of its inner tiles
    shape = lambda w: (TS.grid_of(w, 1).ximages, TS.grid_of(w, 1).yimages)
    assert sorted(shape(2)) == [1, 2] and shape(4) == (2, 2) and shape(8) == (4, 2)
    seams = lambda g: 4 - sum((g.west_boundary, g.east_boundary, g.south_boundary, g.north_boundary))
    assert {seams(TS.grid_of(8, im)) for im in range(1, 9)} == {2, 3}
    assert {(g.its - g.ims, g.ime - g.ite) for g in (TS.grid_of(4, im, 2) for im in range(1, 5))} == {(1, 2), (2, 1)}, "halo width 2: the two sides of a tile differ"


def test_every_tile_has_land_and_water(th_oracle, tab):
    for name in ("ysu+bmj", "noah+ysu"):
        c, _, _ = TS.whole_case(th_oracle, TS.CONFIGS[name], tab)
        for world in WORLDS:
            for halo in (1, 2):
                for image in range(1, world + 1):
                    _, gl = TS.owned(TS.grid_of(world, image, halo))
                    lm = c["land_mask"][gl]
                    assert (lm == 1).any() and (lm == 2).any(), (name, world, halo, image)


@pytest.mark.parametrize("name", ["ysu+bmj", "simple+tiedtke", "ysu+nsas+mpdata", "ysu+nsas@h2"])
def test_every_tile_convects(runs, name):
    for world in WORLDS:
        chains, counts, _ = runs(name, world)
        assert counts == [3, 3]
        per_tile = [sum(ch.convecting) for ch in chains]
        print(name, "world", world, "convecting columns per tile, summed over the sub-steps:", per_tile)
        assert min(per_tile) > 0, (name, world, per_tile)
        assert all((ch.acc[TS.owned(ch.g)[0]] > 0).any() for ch in chains), "it rains in every tile"


@pytest.mark.parametrize("name", list(TS.CONFIGS))
def test_gate_clock_and_dt(runs, th_oracle, name):
    one, counts1, clocks1 = runs(name, 1)
    for world in WORLDS:
        chains, counts, clocks = runs(name, world)
        assert counts == counts1 and clocks == clocks1 and sum(counts) >= 4, "the tiled run takes the one-image run's steps"
        for ch in chains:
            g = ch.gates
            assert len(g) == sum(counts) and g[0] and False in g and True in g[g.index(False):], f"the gate: open, shut, open again: {g}"
    # co_min has something to decide: at the start the images' own steps differ and the smallest is the whole domain's, under the cap
    cfg = TS.CONFIGS[name]
    c = one[0].c                                                         # the one image's cut is the whole domain as it starts
    fresh = [TS.first_dt(th_oracle, TS.cut(c, TS.grid_of(4, im, cfg["halo"]))) for im in range(1, 5)]
    assert len(set(fresh)) > 1 and min(fresh) == TS.first_dt(th_oracle, c) < 120.0, fresh


def test_pbl_simple_is_row_coupled_on_this_case(runs):
    one = runs("simple+tiedtke", 1)[0][0]
    for world in WORLDS:
        chains = runs("simple+tiedtke", world)[0]
        rows = 0
        for ch in chains:
            lo, gl = TS.owned(ch.g)
            rows += sum(int((a[lo[0]] != b[gl[0]]).sum()) for a, b in zip(ch.pbl_rows, one.pbl_rows))
        n = differing(chains, one)
        print("world", world, "tile rows whose nsubsteps differ from the whole row's:", rows, "owned cells of theta that differ:", n)
        assert rows > 0 and n > 0, (world, rows, n)


def test_nsas_is_row_coupled_on_this_case(runs):
    one = runs("ysu+nsas@h2", 1)[0][0]
    for world in WORLDS:
        chains = runs("ysu+nsas@h2", world)[0]                           # upwind: nothing but NSAS can tell the tiling
        rows = sum(int((ch.cu["limits"][TS.owned(ch.g)[0][0]] != one.cu["limits"][TS.owned(ch.g)[1][0]]).any(axis=1).sum()) for ch in chains)
        n = differing(chains, one)
        print("world", world, "tile rows whose kbmax / kbm / kmax differ from the whole row's:", rows, "owned cells of theta that differ:", n)
        assert rows > 0 and n > 0, (world, rows, n)
        assert differing(runs("ysu+nsas+mpdata", world)[0], runs("ysu+nsas+mpdata", 1)[0][0]) > 0


def test_tiedtke_row_differs_through_pbl_simple_and_not_through_leveltop(runs):
    """see the module's docstring"""
    alone = dict(TS.CONFIGS["simple+tiedtke"], pbl="ysu")
    one = runs("ysu+tiedtke", 1, alone)[0][0]
    assert sum(one.convecting) > 0
    for world in WORLDS:
        assert differing(runs("simple+tiedtke", world)[0], runs("simple+tiedtke", 1)[0][0]) > 0
        for field in TS.SCALARS + ["acc"]:
            assert differing(runs("ysu+tiedtke", world, alone)[0], one, field) == 0, (world, field)


@pytest.mark.parametrize("name", [n for n, c in TS.CONFIGS.items() if c["star"]])
def test_star_configurations_do_not_see_the_tiling(runs, name):
    cfg = TS.CONFIGS[name]
    one = runs(name, 1)[0][0]
    want = TS.chain_fields(cfg, one)
    for world in WORLDS:
        for ch in runs(name, world)[0]:
            lo, gl = TS.owned(ch.g)
            got = TS.chain_fields(cfg, ch)
            for group in got:
                for k, a in got[group].items():
                    assert TS.nbits(TS.own(a, lo), TS.own(want[group][k], gl)) == 0, (name, world, group, k)

"""Thompson and mp_simple where their launch layout changes, against the CPU oracle in the reference's own math, bit for bit.

The layout is a function of the level count alone (icar_amd/csrc/column_comm.h): k_thompson_lane (one column per wave) at 57..64
levels and at 1; k_thompson_pack<512> with 256- or 512-thread blocks; k_thompson_pack<1024> -- which 37, 43 and 44 levels get, not
only tall columns; level masks up to 64 levels and flag words above; 1 .. 128 columns per block.  tests/test_mp_columns_inputs.py
holds the table and shows, without a GPU, that the heights below reach every row of it and that the inputs exercise the exchanges
(carried fall speeds over several levels and across level 63 / 64, sub-step counts that differ inside a block).
  * every height from 1 to 130 levels and both ends of every row of the table up to 1024, Thompson and mp_simple; 1025 is refused;
  * process_halo's strips in one launch at one height of each kind, 1- and 2-wide; a launch of more blocks than one XCD turn;
  * configs[4]'s 80 levels at size: 512 x 512 x 80 and its 8-GPU tile 256 x 128 x 80."""
import ctypes
import numpy as np
import pytest
from icar_amd.capi import lib, check
from icar_amd.options import options_t
from icar_amd.microphysics import mp, mp_init, mp_tiles
from icar_amd.constants import kMP_THOMPSON, kMP_SB04
from util import single_image_domain, bits_equal, nbitdiff
import mp_columns_case as M
from test_gpu_thompson import FIELDS, EXACT, check_close, run_case

pytestmark = pytest.mark.gpu
ACC = {"acc_rain": "accumulated_precipitation", "acc_snow": "accumulated_snowfall", "acc_graupel": "graupel"}


def sweep(run, heights):
    """run(nk) at every height; the heights that fail, and how, in one message"""
    bad = {}
    for nk in heights:
        try:
            run(nk)
        except (AssertionError, RuntimeError) as e:
            bad[nk] = str(e).splitlines()[0][:200]
    assert not bad, f"{len(bad)} of {len(heights)} column heights fail: " + "; ".join(f"nk={k}: {v}" for k, v in bad.items())


def same_bits(got, ref, what):
    """every field of ref: the device's bits.  (The accumulators are REAL(8): equal values, no NaN)"""
    for k in ref:
        if ref[k].dtype == np.float64:
            assert got[k].dtype == np.float64 and np.array_equal(got[k], ref[k]), f"{what} {k}: {(got[k] != ref[k]).sum()} of {ref[k].size} columns differ"
        else:
            assert bits_equal(got[k], ref[k]), (f"{what} {k}: {nbitdiff(got[k], ref[k])} of {ref[k].size} cells differ, first at (j, k, i) = "
                                                f"{tuple(int(x[0]) for x in np.nonzero(got[k].view(np.int32) != ref[k].view(np.int32)))}")


def thompson_device_run(c, dt, calls=M.CALLS, cool=M.COOL, launch=None):
    """`calls` microphysics calls of the device on the case, cooled between them like M.thompson_oracle_run.  launch(d, g): the
    Thompson call to make instead of mp(d, opt, dt)"""
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.microphysics = kMP_THOMPSON
        mp_init(opt, d)
        for _ in range(calls):
            if launch is None:
                mp(d, opt, dt)
            else:
                launch(d, d.grid)
            d.model_time_seconds += dt
            d.set("potential_temperature", d.get("potential_temperature") - np.float32(cool))
        out = {k: d.get(m) for k, m in FIELDS.items()}
        out.update({k: d.get(m) for k, m in ACC.items()})
        return out
    finally:
        d.close()


def thompson_height(th_oracle, probe, nk):
    kind, nt, cpb = M.launch_geometry(probe, nk)[:3]
    c = M.thompson_case(probe, nk)
    dt = M.thompson_dt(nk)
    ref, plans = M.thompson_oracle_run(th_oracle, c, dt, levels=M.SINGLE_LEVEL if nk == 1 else None)
    M.check_thompson_oracle(c, ref, plans, kind, cpb)
    launch = None
    if nk == 1:                                        # a context holds at least two levels: one level is kts = kte of a taller tile
        def launch(d, g):
            check(lib().icar_hip_thompson(d.ctx, ctypes.c_float(dt), g.its, g.ite, g.jts, g.jte, M.SINGLE_LEVEL, M.SINGLE_LEVEL,
                                          g.ids, g.ide, g.jds, g.jde, g.kds, g.kde), "thompson")
    got = thompson_device_run(c, dt, launch=launch)
    same_bits(got, ref, f"nk={nk} ({M.KIND[kind]} {nt} threads, {cpb} columns per block)")
    assert M.untouched(c, got), "the ring or the last global row / column changed on the device"


def test_thompson_every_column_height(th_oracle, probe):
    """Thompson at every height of M.HEIGHTS on a narrow tile (a partial block at each end of a row, two full ones between, three
    rows) of layered hydrometeors, six calls with cooling between them: the oracle-side conditions of the height
    (M.check_thompson_oracle), then all nine fields and the three accumulators bit-identical to the oracle, the ring and the last
    global row and column bit-identical to the input.  nk = 1 included (kts = kte = 2 of a three-level tile, as a context holds at
    least two levels): the lane kernel with one busy lane (ksed1 = kte - 1 = -1, nothing falls between levels), judged by the oracle
    like the others; the levels below and above it stay as they are."""
    sweep(lambda nk: thompson_height(th_oracle, probe, nk), M.HEIGHTS)


def test_thompson_refuses_more_than_1024_levels(probe):
    """1025 levels: the library's error, no launch, and the fields stay as they were"""
    nk = M.TOO_TALL
    assert M.launch_geometry(probe, nk)[0] == 0
    c = M.make_case(nk, 7, 5)
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.microphysics = kMP_THOMPSON
        mp_init(opt, d)
        with pytest.raises(RuntimeError, match="levels are not supported"):
            mp(d, opt, 60.0)
        for k, m in FIELDS.items():
            assert bits_equal(d.get(m), c[k]), k
    finally:
        d.close()


# ---- process_halo's strips in one launch -----------------------------------------------------------------------------------------
def strips_case(probe, nk, simple=False):
    """a tile whose ring strips end in partial blocks: neither nx nor the strips' lengths along j (ny - 2 rows, ny - 4 between the
    corners) are multiples of the columns per block"""
    g = M.launch_geometry(probe, nk)
    group = g[4] if simple else (g[2] if g[0] == M.PACK else 4)
    nx = 2 * group + group // 2 + 4; ny = 2 * group + group // 2 + 5
    if group > 1:
        nx = next(n for n in range(nx, nx + group) if n % group)
        ny = next(n for n in range(ny, ny + 2 * group) if (n - 2) % group and ((n - 4) % group or group == 2))
    return M.make_case(nk, nx, ny, species=("rain", "snow") if simple else ("rain", "cloud_ice", "snow", "graupel"), hill=3000.0 if simple else 1000.0)


def thompson_tiles_launch(tiles, dt, batched):
    def launch(d, g):
        if batched:
            arr = ((ctypes.c_int * 4) * 4)(*[(ctypes.c_int * 4)(*t) for t in tiles])
            check(lib().icar_hip_thompson_tiles(d.ctx, ctypes.c_float(dt), len(tiles), arr, g.kts, g.kte, g.ids, g.ide, g.jds, g.jde, g.kds, g.kde), "thompson_tiles")
        else:
            for (a, b, cc, dd) in tiles:
                check(lib().icar_hip_thompson(d.ctx, ctypes.c_float(dt), a, b, cc, dd, g.kts, g.kte, g.ids, g.ide, g.jds, g.jde, g.kds, g.kde), "thompson")
    return launch


@pytest.mark.parametrize("nk,halo", [(60, 1), (80, 1), (12, 1), (65, 1), (43, 1), (105, 1), (43, 2), (80, 2)])
def test_thompson_halo_strips_other_geometries(th_oracle, probe, nk, halo):
    """The four strips of process_halo in one launch == four launches == the oracle on the same strips, bit for bit, three calls:
    the lane kernel (60 levels), 256-thread blocks of 3 and of 21 columns (80, 12), 512 threads (65), 1024 threads below and above
    64 levels (43, 105).  halo = 1: the west / east strips are one column wide and pack along j (`tall`), ending in a partial block;
    halo = 2: they are two wide and pack along i."""
    c = strips_case(probe, nk)
    nx, ny = c["nx"], c["ny"]
    dt = M.thompson_dt(nk)
    tiles = mp_tiles(2, nx - 1, 2, ny - 1, halo=halo)
    assert len(tiles) == 4 and all((b - a + 1 == halo) != (dd - cc + 1 == halo) for (a, b, cc, dd) in tiles), tiles
    ref, _ = M.thompson_oracle_run(th_oracle, c, dt, calls=3, tiles=tiles, diag=False)
    inner = (slice(1 + halo, -1 - halo), slice(None), slice(1 + halo, -1 - halo))
    assert (ref["cloud_water"] != c["cloud_water"]).any() and np.array_equal(ref["rain"][inner], c["rain"][inner]), "only the strips are processed"
    one = thompson_device_run(c, dt, calls=3, launch=thompson_tiles_launch(tiles, dt, True))
    four = thompson_device_run(c, dt, calls=3, launch=thompson_tiles_launch(tiles, dt, False))
    same_bits(one, ref, f"nk={nk} halo={halo}: one launch vs oracle:")
    same_bits(four, ref, f"nk={nk} halo={halo}: four launches vs oracle:")


def test_thompson_more_blocks_than_one_xcd_turn(th_oracle):
    """The XCD-aware block order of k_thompson_pack permutes the block ids inside whole super-runs of 8 x 64 blocks and leaves the
    tail as it is.  200 x 40 x 40: 34 blocks per row x 38 rows = 1292 = 2 x 512 + 268 blocks, so both ranges compute columns; the
    whole tile against the oracle, two calls."""
    out, ref = run_case(th_oracle, mode=0, nx=200, ny=40, nz=40, steps=2, cool=1.5, moist=2.0, dt=60.0)
    assert ref["rain"].max() > 1e-6
    check_close(out, ref, rtol=1e-5, label="xcd_tail_200x40x40/mode0", **EXACT)


# ---- configs[4]: 80 levels at size -------------------------------------------------------------------------------------------------
def test_thompson_config4_80_levels_full_size(th_oracle):
    """configs[4]'s grid, 512 x 512 x 80 (256-thread blocks of 3 columns, flag words), two microphysics calls on the moistened
    ideal hill: every column bit for bit.  (Measured on 16 CPUs beside an MI355X: 6 s for the whole test, the oracle's two calls over all 262 144 columns included.)"""
    out, ref = run_case(th_oracle, mode=0, nx=512, ny=512, nz=80, steps=2, cool=1.5, moist=1.8, dt=60.0, uniform_dz=160.0)
    assert ref["rain"].max() > 1e-5 and ref["cloud_water"].max() > 1e-5 and ref["acc_rain"].max() > 0
    check_close(out, ref, rtol=1e-5, label="config4_512x512x80/mode0", **EXACT)


def test_thompson_config4_80_levels_tile_layered(th_oracle):
    """configs[4]'s 8-GPU tile, 256 x 128 x 80, with the layered hydrometeors of the height sweep, two calls: every column bit for bit"""
    c = M.make_case(80, 256, 128)
    dt = M.thompson_dt(80)
    ref, plans = M.thompson_oracle_run(th_oracle, c, dt, calls=2)
    M.check_thompson_oracle(c, ref, plans, M.PACK, 3)
    same_bits(thompson_device_run(c, dt, calls=2), ref, "256x128x80 layered")


# ---- mp_simple -----------------------------------------------------------------------------------------------------------------------
def simple_device_run(c, dt, calls=M.SIMPLE_CALLS, cool=M.SIMPLE_COOL, top=None, halo=None):
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.microphysics = kMP_SB04
        if top is not None:
            opt.mp_options.top_mp_level = top
        mp_init(opt, d)
        for _ in range(calls):
            if halo is not None:                       # the halo pass leaves last_model_time to the interior pass (mp_driver.f90:711):
                check(lib().icar_hip_mp_reset(d.ctx), "mp_reset")      # without one, start each call over so that its mp_dt is dt
            mp(d, opt, dt, halo=halo)
            d.model_time_seconds += dt
            d.set("potential_temperature", d.get("potential_temperature") - np.float32(cool))
        out = {k: d.get(m) for k, m in M.SIMPLE_OUT.items()}
        out["acc_rain"] = d.get("accumulated_precipitation"); out["acc_snow"] = d.get("accumulated_snowfall")
        return out
    finally:
        d.close()


def simple_equal(got, ref, what):
    for k in ref:
        assert np.array_equal(got[k], ref[k]), f"{what} {k}: {(got[k] != ref[k]).sum()} of {ref[k].size} differ"
        import util
        util.COUNTS["bit_exact_fields"] += 1


def simple_height(oracle, probe, nk):
    nt, cpb = M.launch_geometry(probe, nk)[3:]
    c = M.simple_case(probe, nk)
    dt = M.simple_dt(nk)
    ref = M.simple_oracle_run(oracle, c, dt)
    M.check_simple_oracle(c, ref, dt, cpb)
    simple_equal(simple_device_run(c, dt), ref, f"nk={nk} ({nt} threads, {cpb} columns per block)")


def test_mp_simple_every_column_height(oracle, probe):
    """k_mp_simple_pack through mp() at every height of M.HEIGHTS but 1 (its columns are the context's, which holds at least two
    levels; it takes block_comm_geometry() as it comes: 256-, 512- and
    1024-thread blocks of 1 .. 256 columns): layered rain and snow over a 3 km hill, four calls with cooling between them, a time
    step for which rain's sub-step count differs between the columns of a block; the oracle-side conditions
    (M.check_simple_oracle), then every field and both accumulators equal to the oracle's."""
    sweep(lambda nk: simple_height(oracle, probe, nk), M.SIMPLE_HEIGHTS)


def test_mp_simple_refuses_more_than_1024_levels(probe):
    nk = M.TOO_TALL
    assert M.launch_geometry(probe, nk)[3] == 0
    c = M.make_case(nk, 7, 5, species=("rain", "snow"))
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.microphysics = kMP_SB04
        mp_init(opt, d)
        with pytest.raises(RuntimeError, match="more than 1024 levels"):
            mp(d, opt, 5.0)
    finally:
        d.close()


def test_a_context_of_one_level_is_refused():
    """why the sweeps reach one level only through kts = kte: icar_hip_ctx_create takes tiles of two levels and more"""
    with pytest.raises(RuntimeError, match="at least"):
        single_image_domain(M.make_case(1, 7, 5, species=("rain", "snow"))).close()


@pytest.mark.parametrize("nk", [30, 56, 105])
def test_mp_simple_top_mp_level_below_the_column_top(oracle, probe, nk):
    """top_mp_level five levels below the column top, one height per block size (256, 512, 1024 threads): the conversions stop
    there (`in_k`), the fall from above it does not (`top`); equal to the oracle run with that kte, and the levels above unchanged
    but for what falls out of them"""
    nt = M.launch_geometry(probe, nk)[3]
    assert nt == {30: 256, 56: 512, 105: 1024}[nk]
    top = nk - 5
    c = M.simple_case(probe, nk)
    dt = M.simple_dt(nk)
    ref = M.simple_oracle_run(oracle, c, dt, top=top)
    full = M.simple_oracle_run(oracle, c, dt)
    assert not np.array_equal(ref["water_vapor"], full["water_vapor"]), "top_mp_level must matter in this case"
    simple_equal(simple_device_run(c, dt, top=top), ref, f"nk={nk} top_mp_level={top}")


@pytest.mark.parametrize("nk", [43, 80])
def test_mp_simple_halo_strips_other_geometries(oracle, probe, nk):
    """mp(halo=1): process_halo's four strips go through one launch of k_mp_simple_pack (blockIdx.z = strip); equal to the oracle
    on the same four strips at 43 levels (1024-thread blocks of 23 columns) and 80 (256-thread blocks of 3)"""
    c = strips_case(probe, nk, simple=True)
    nx, ny = c["nx"], c["ny"]
    dt = M.simple_dt(nk)
    tiles = mp_tiles(2, nx - 1, 2, ny - 1, halo=1)
    ref = M.simple_oracle_run(oracle, c, dt, calls=3, tiles=tiles)
    assert (ref["rain"] != c["rain"]).any() and np.array_equal(ref["rain"][2:-2, :, 2:-2], c["rain"][2:-2, :, 2:-2]), "only the strips are processed"
    simple_equal(simple_device_run(c, dt, calls=3, halo=1), ref, f"nk={nk} strips")

"""WSM3 and WSM6 on the device at every column height they accept (3 / 4 .. 64 levels), against the CPU oracle in the reference's own
math (mode 0), bit for bit.  Up to 63 levels the semi-Lagrangian fall runs one wave per column (16-column LDS tiles, for WSM3 inside
64-column x blocks), at 64 one thread per column.  tests/wsm_columns_case.py holds the inputs, tests/test_wsm_columns_inputs.py
shows without a GPU that they reach every branch of the fall at every height, tests/test_oracle_wsm_columns.py holds the oracle to
the compiled reference on the same inputs, tests/test_gpu_wsm_fall.py compares the fall alone.
  * every height, two states (rain to the model top; snow and graupel at the ground), three calls with cooling, a tile of 83 x 3
    columns: five full 16-column tiles and one of three columns, a partial second 64-column block;
  * process_halo's strips 1 and 2 wide, strips + interior on two streams, WSM6's four strips in one launch against four;
  * tiles 1 .. 17, 31 .. 33, 63 .. 65 columns wide through icar_hip_wsm3 / icar_hip_wsm6;
  * a level sub-range (kts = kms + 2, kte = kme - 3) in the wave form and in the serial form;
  * heights outside the range are refused by the library's argument check, launch nothing and leave the context usable;
  * the serial form with snow and graupel at the ground over two minor loops."""
import ctypes
import numpy as np
import pytest
from icar_amd.capi import lib, check
from icar_amd.options import options_t
from icar_amd.microphysics import mp, mp_init, mp_var_request, mp_tiles
from icar_amd.constants import kMP_WSM3, kMP_WSM6
from util import single_image_domain, bits_equal, nbitdiff
import wsm_columns_case as W

pytestmark = pytest.mark.gpu
NAMES = {"cloud_water": "cloud_water_mass", "rain": "rain_mass", "cloud_ice": "cloud_ice_mass", "snow": "snow_mass", "graupel": "graupel_mass"}
ACC = {"acc_rain": "accumulated_precipitation", "acc_snow": "accumulated_snowfall", "acc_graupel": "graupel"}
RANGE = {3: "3..64 levels", 6: "4..64 levels"}


def sweep(run, heights):
    """run(nk) at every height; the heights that fail, and how, in one message"""
    bad = {}
    for nk in heights:
        try:
            run(nk)
        except (AssertionError, RuntimeError) as e:
            bad[nk] = str(e).splitlines()[0][:240]
    assert not bad, f"{len(bad)} of {len(heights)} column heights fail: " + "; ".join(f"nk={k}: {v}" for k, v in bad.items())


def same_bits(got, ref, what):
    """every field of ref: the device's bits.  (The accumulators are REAL(8): equal values, no NaN)"""
    for k in ref:
        if ref[k].dtype == np.float64:
            assert got[k].dtype == np.float64 and np.array_equal(got[k], ref[k]), f"{what} {k}: {(got[k] != ref[k]).sum()} of {ref[k].size} columns differ"
        else:
            assert bits_equal(got[k], ref[k]), (f"{what} {k}: {nbitdiff(got[k], ref[k])} of {ref[k].size} cells differ, first at (j, k, i) = "
                                                f"{tuple(int(x[0]) for x in np.nonzero(got[k].view(np.int32) != ref[k].view(np.int32)))}")


def open_domain(scheme, c):
    d = single_image_domain(c)
    if scheme == 3:
        d.set("w_real", c["w_real"])
    opt = options_t(); opt.physics.microphysics = kMP_WSM3 if scheme == 3 else kMP_WSM6
    mp_var_request(opt); mp_init(opt, d)
    return d, opt


def fields(scheme, d):
    out = {k: d.get(NAMES.get(k, k)) for k in W.KEYS[scheme]}
    out.update({k: d.get(m) for k, m in ACC.items() if scheme == 6 or k != "acc_graupel"})
    return out


def direct(scheme, dt, tiles, kts, kte, batched=False):
    """launch(d, opt): the scheme's own entry point on each tile (batched: WSM6's four tiles in one call)"""
    def launch(d, opt):
        if batched:
            arr = ((ctypes.c_int * 4) * 4)(*[(ctypes.c_int * 4)(*t) for t in tiles])
            check(lib().icar_hip_wsm6_tiles(d.ctx, ctypes.c_float(dt), len(tiles), arr, kts, kte), "wsm6_tiles")
        else:
            fn = lib().icar_hip_wsm3 if scheme == 3 else lib().icar_hip_wsm6
            for (a, b, cc, dd) in tiles:
                check(fn(d.ctx, ctypes.c_float(dt), a, b, cc, dd, kts, kte), f"wsm{scheme}")
    return launch


def device_run(scheme, c, dt, calls=W.CALLS, cool=0.0, launch=None):
    """`calls` microphysics calls of the device on the case, cooled between them like W.oracle_run.  launch(d, opt): the call to make
    instead of mp(d, opt, dt)"""
    d, opt = open_domain(scheme, c)
    try:
        for _ in range(calls):
            if launch is None:
                mp(d, opt, dt)
            else:
                launch(d, opt)
            d.model_time_seconds += dt
            d.set("potential_temperature", d.get("potential_temperature") - np.float32(cool))
        return fields(scheme, d)
    finally:
        d.close()


def scheme_height(oracle, scheme, nk):
    for state, s in W.STATES.items():
        c = W.make_case(scheme, nk, state)
        dt = W.wsm_dt(nk)
        ref = W.oracle_run(oracle, scheme, c, dt, state=state)
        assert ref["acc_rain"].max() > 0 and (state == "warm" or ref["acc_snow"].max() > 0.05)
        got = device_run(scheme, c, dt, cool=s["cool"])
        same_bits(got, ref, f"nk={nk} {state}")
        assert W.untouched(c, got, scheme, cool=s["cool"]), f"nk={nk} {state}: the ring outside its .. ite, jts .. jte changed on the device"


def test_wsm3_every_column_height(oracle):
    """WSM3 through mp() at 3 .. 64 levels: all four fields and both REAL(8) accumulators bit-identical to the oracle, the ring
    byte-identical to the input"""
    sweep(lambda nk: scheme_height(oracle, 3, nk), W.WSM3_HEIGHTS)


def test_wsm6_every_column_height(oracle):
    """WSM6 through mp() at 4 .. 64 levels: all seven fields and the three REAL(8) accumulators bit-identical to the oracle, the ring
    byte-identical to the input"""
    sweep(lambda nk: scheme_height(oracle, 6, nk), W.WSM6_HEIGHTS)


# ---- strips ----------------------------------------------------------------------------------------------------------------------
STRIP_HEIGHTS = [5, 40, 62, 63, 64]                     # short; the widest tested before; both sides of the wave / serial switch


@pytest.mark.parametrize("halo", [1, 2])
@pytest.mark.parametrize("nk", STRIP_HEIGHTS)
@pytest.mark.parametrize("scheme", [3, 6])
def test_strips_and_interior_equal_the_whole_tile(oracle, scheme, nk, halo):
    """mp(halo) + mp(subset) -- and, one column wide, mp_and_halo's two streams -- == the oracle on the whole tile"""
    c = W.make_case(scheme, nk, "cold", nx=43, ny=12)
    dt = W.wsm_dt(nk); cool = W.STATES["cold"]["cool"]
    ref = W.oracle_run(oracle, scheme, c, dt, state="cold")

    def split(d, opt):
        mp(d, opt, dt, halo=halo); mp(d, opt, dt, subset=halo)
    same_bits(device_run(scheme, c, dt, cool=cool, launch=split), ref, f"wsm{scheme} nk={nk} halo={halo}: strips + interior:")
    if halo == 1:
        from icar_amd.time_step import mp_and_halo
        same_bits(device_run(scheme, c, dt, cool=cool, launch=lambda d, opt: mp_and_halo(d, opt, dt)), ref, f"wsm{scheme} nk={nk}: two streams:")


@pytest.mark.parametrize("halo", [1, 2])
@pytest.mark.parametrize("nk", STRIP_HEIGHTS)
def test_wsm6_four_strips_in_one_launch(oracle, nk, halo):
    """process_halo's four strips as one icar_hip_wsm6_tiles call == four icar_hip_wsm6 calls == the oracle on the same strips; the
    interior stays as it was"""
    c = W.make_case(6, nk, "cold", nx=43, ny=12)
    nx, ny = c["nx"], c["ny"]
    dt = W.wsm_dt(nk); cool = W.STATES["cold"]["cool"]
    tiles = mp_tiles(2, nx - 1, 2, ny - 1, halo=halo)
    assert len(tiles) == 4 and all((b - a + 1 == halo) != (dd - cc + 1 == halo) for (a, b, cc, dd) in tiles), tiles
    ref = W.oracle_run(oracle, 6, c, dt, state="cold", tiles=tiles)
    assert W.untouched(c, ref, 6, cool=cool, tiles=tiles) and (ref["rain"] != c["rain"]).any()
    one = device_run(6, c, dt, cool=cool, launch=direct(6, dt, tiles, 1, nk, batched=True))
    four = device_run(6, c, dt, cool=cool, launch=direct(6, dt, tiles, 1, nk))
    same_bits(one, ref, f"nk={nk} halo={halo}: one launch:")
    same_bits(four, ref, f"nk={nk} halo={halo}: four launches:")


# ---- tile widths -----------------------------------------------------------------------------------------------------------------
WIDTHS = list(range(1, 18)) + [31, 32, 33, 63, 64, 65]


@pytest.mark.parametrize("nk", [40, 63])
@pytest.mark.parametrize("scheme", [3, 6])
def test_tile_widths(oracle, scheme, nk):
    """a tile of every width of WIDTHS, each on a row of its own (its = 2, 3 or 4), through the scheme's own entry point, two passes:
    the whole state equal to the oracle on the same tiles, the columns outside them untouched"""
    c = W.make_case(scheme, nk, "cold", nx=70, ny=len(WIDTHS) + 2)
    tiles = [(2 + w % 3, 2 + w % 3 + w - 1, 2 + n, 2 + n) for n, w in enumerate(WIDTHS)]
    assert max(t[1] for t in tiles) <= c["nx"] - 1 and sorted(t[1] - t[0] + 1 for t in tiles) == WIDTHS
    dt = W.wsm_dt(nk); cool = W.STATES["cold"]["cool"]
    ref = W.oracle_run(oracle, scheme, c, dt, calls=2, state="cold", tiles=tiles)
    assert W.untouched(c, ref, scheme, calls=2, cool=cool, tiles=tiles)
    got = device_run(scheme, c, dt, calls=2, cool=cool, launch=direct(scheme, dt, tiles, 1, nk))
    same_bits(got, ref, f"wsm{scheme} nk={nk} widths:")
    assert W.untouched(c, got, scheme, calls=2, cool=cool, tiles=tiles), "a column outside the tiles changed on the device"


# ---- a level sub-range -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,form", [(45, "wave"), (69, "serial")])
@pytest.mark.parametrize("scheme", [3, 6])
def test_level_sub_range(oracle, scheme, nz, form):
    """kts = kms + 2, kte = kme - 3 (k0 = 2) through the scheme's own entry point: 40 of 45 levels (wave form) and 64 of 69 (serial
    form) equal to the oracle on the same range; the levels outside keep their bytes"""
    kts, kte = 3, nz - 3
    assert (kte - kts + 1 <= 63) == (form == "wave") and kte - kts + 1 in (40, 64)
    c = W.make_case(scheme, nz, "cold")
    tile = (2, c["nx"] - 1, 2, c["ny"] - 1)
    dt = W.wsm_dt(nz); cool = W.STATES["cold"]["cool"]
    ref = W.oracle_run(oracle, scheme, c, dt, state="cold", levels=(kts, kte))
    assert W.untouched(c, ref, scheme, cool=cool, levels=(kts, kte)) and ref["acc_rain"].max() > 0
    got = device_run(scheme, c, dt, cool=cool, launch=direct(scheme, dt, [tile], kts, kte))
    same_bits(got, ref, f"wsm{scheme} levels {kts}..{kte} of {nz}:")
    assert W.untouched(c, got, scheme, cool=cool, levels=(kts, kte)), "a level outside kts .. kte changed on the device"


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,nz,levels,valid", [(3, 12, (1, 2), (1, 12)), (6, 12, (1, 3), (1, 12)), (3, 69, (1, 65), (3, 66)), (6, 69, (1, 65), (3, 66)),
                                                    (3, 65, None, (1, 64)), (6, 65, None, (2, 65))])
def test_heights_outside_the_range_are_refused(oracle, scheme, nz, levels, valid):
    """WSM3 at 2 and 65 levels, WSM6 at 3 and 65 (levels = None: the whole 65-level context through mp()): the library's argument
    check answers with the accepted range and launches nothing -- every field and accumulator keeps its bytes -- and the context
    serves a following valid call, which equals the oracle"""
    c = W.make_case(scheme, nz, "cold", nx=24)
    tile = (2, c["nx"] - 1, 2, c["ny"] - 1)
    dt = W.wsm_dt(min(nz, 64))
    d, opt = open_domain(scheme, c)
    try:
        for k, m in ACC.items():                               # (the library creates the accumulators with the first launch: put them there)
            if scheme == 6 or k != "acc_graupel":
                d.set(m, np.zeros((c["ny"], c["nx"]), np.float64))
        with pytest.raises(RuntimeError, match=RANGE[scheme].replace(".", r"\.")):
            if levels is None:
                mp(d, opt, dt)
            else:
                direct(scheme, dt, [tile], *levels)(d, opt)
        before = fields(scheme, d)
        for k in W.KEYS[scheme]:
            assert bits_equal(before[k], c[k]), f"{k} changed by a refused call"
        assert all(not before[a].any() for a in before if a.startswith("acc_"))
        direct(scheme, dt, [tile], *valid)(d, opt)
        got = fields(scheme, d)
    finally:
        d.close()
    ref = W.oracle_run(oracle, scheme, c, dt, calls=1, cool=0.0, levels=valid)
    same_bits(got, ref, f"wsm{scheme} levels {valid} after a refused call:")


# ---- the serial form with substance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [3, 6])
def test_serial_form_64_levels_cold_two_minor_loops(oracle, scheme):
    """64 levels (one thread per column), the cold state, 240 s = two minor loops of 120 s, four calls on 83 x 6 columns: snow (for
    WSM6 graupel too) reaches the ground in amounts, every field and accumulator equal to the oracle"""
    c = W.make_case(scheme, 64, "cold", ny=8)
    dt = W.wsm_dt(64); cool = W.STATES["cold"]["cool"]
    assert dt == 240.0
    ref = W.oracle_run(oracle, scheme, c, dt, calls=4, state="cold")
    assert ref["acc_rain"].max() > 1.0 and ref["acc_snow"].max() > 0.5 and (scheme == 3 or ref["acc_graupel"].max() > 0.5)
    assert np.count_nonzero(ref["acc_snow"]) > 0.8 * 83 * 6
    got = device_run(scheme, c, dt, calls=4, cool=cool)
    same_bits(got, ref, f"wsm{scheme} 64 levels cold:")

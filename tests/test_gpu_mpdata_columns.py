"""MPDATA where its launch layout changes and where float32 runs out of range, against the CPU oracle (bit-exact restatement of the
compiled reference):
  * every column height from 2 to 120 levels.  The fused kernel (mpdata.hip) cuts a column into level ranges, waves and levels per
    thread by nz alone, so each height is its own layout: 1..5 levels per thread, 5..8 waves, idle levels in the top wave, 1..4
    level ranges with halo levels, waves above the column top.  Each height runs the fused kernel (every cell within the gate and its
    0.3 margin), the exact mode (bit for bit; it takes 3 levels and more), the donor-cell pass inside the fused kernel (bit for bit)
    and the third-order form with advect_density.  (nz = 2 without the limiter only: adv_mpdata_FCT_core.f90 reads q1(i+2) of a
    2-cell line.)
  * configs[4]'s 80 levels at size: 512 x 512 x 80 and its 8-GPU tile 256 x 128 x 80 with rough winds.
  * fields near the bottom of the float range: normal numbers just above FLT_MIN whose fluxes are subnormal, fields that are subnormal
    throughout, and cloud edges where such values sit next to 1e-4."""
import numpy as np
import pytest
from icar_amd import ideal
from icar_amd.options import options_t
from icar_amd.advection import advect, setup_winds
from icar_amd.capi import lib, check
from icar_amd.constants import kADV_UPWIND, kADV_MPDATA
from util import (SCALARS, MEMBER, KVAR, MPDATA_RTOL, MPDATA_MARGIN, bits_equal, nbitdiff, single_image_domain, adv_args, assert_fields_close,
                  roughen_winds)
from mpdata_rows_case import column_case          # (the tile of these sweeps; the horizontal sweeps build theirs from it)

pytestmark = pytest.mark.gpu

NAMES = ["water_vapor", "cloud_water", "potential_temperature"]
HEIGHTS = range(2, 121)


def device_advect(c, names, dt, dens=False, order=2, fct=True, nsteps=1, exact_mode=False, scheme=kADV_MPDATA):
    d = single_image_domain(c)
    if exact_mode:
        check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    opt = options_t()
    opt.physics.advection = scheme; opt.parameters.advect_density = dens
    opt.adv_options.mpdata_order = order; opt.adv_options.flux_corrected_transport = fct
    opt.advect_vars([KVAR[n] for n in names])
    try:
        for _ in range(nsteps):
            advect(d, opt, dt)
        return {n: d.get(MEMBER[n]) for n in names}
    finally:
        d.close()


def oracle_advect(oracle, c, names, dt, dens=False, order=2, fct=True, nsteps=1, scheme=kADV_MPDATA):
    q = np.stack([c[n] for n in names]).copy()
    oracle.advect(scheme, q, *adv_args(c), dt, advect_density=dens, mpdata_order=order, fct=fct, nsteps=nsteps)
    return {n: q[m] for m, n in enumerate(names)}


def fused_donor_cell_pass(probe, c, names, dt, fct=True):
    """the fused kernel's output with the antidiffusive coefficients of the context zeroed (tests/support/mpdata_probe.hip): its q2"""
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.adv_options.mpdata_order = 2
        opt.adv_options.flux_corrected_transport = fct
        opt.advect_vars([KVAR[n] for n in names])
        d.configure(opt)
        setup_winds(d, opt, dt)
        assert probe.icar_probe_mpdata_zero_antidiffusion(d.ctx) == 0
        advect(d, opt, dt)                              # (same scheme, dt and density: the coefficients are not rebuilt)
        return {n: d.get(MEMBER[n]) for n in names}
    finally:
        d.close()


def check_bits(got, ref, what):
    for n in ref:
        assert bits_equal(got[n], ref[n]), f"{what} {n}: {nbitdiff(got[n], ref[n])} of {ref[n].size} cells differ, max |d| = {np.abs(got[n].astype(np.float64) - ref[n]).max():.3e}"


def check_close(got, ref, what, record=None):
    for n in ref:
        assert_fields_close(got[n], ref[n], f"{what} {n}", record=None if record is None else ("mpdata_columns", record))


def sweep(run, heights=HEIGHTS, what="column heights", key="nz="):
    """run(nz) at every height (or run(x) at every x of another list: what, key); those that fail, and how, in one message"""
    bad = {}
    for nz in heights:
        try:
            run(nz)
        except (AssertionError, RuntimeError) as e:
            bad[nz] = str(e).splitlines()[0][:200]
    assert not bad, f"{len(bad)} of {len(heights)} {what} fail: " + "; ".join(f"{key}{k}: {v}" for k, v in bad.items())


def test_every_column_height_fused(oracle):
    """The default path, mpdata_order 2 with the limiter: every cell of every scalar within 1e-5 of the local field scale -- and within
    0.3 of that (assert_fields_close) -- at every height; the field changed."""
    def run(nz):
        c = column_case(oracle, nz)
        fct = nz >= 3
        dt = ideal.cfl_dt(c)
        ref = oracle_advect(oracle, c, NAMES, dt, fct=fct)
        got = device_advect(c, NAMES, dt, fct=fct)
        for n in NAMES:
            assert np.abs(got[n] - c[n]).max() > 0, f"{n}: advection did nothing"
        check_close(got, ref, f"nz={nz}")
    sweep(run)


def test_every_column_height_exact_mode(oracle):
    """icar_hip_mpdata_exact: every cell bit-identical to the oracle over two steps at every height it takes (3 and more levels)"""
    def run(nz):
        c = column_case(oracle, nz)
        dt = ideal.cfl_dt(c)
        check_bits(device_advect(c, NAMES, dt, nsteps=2, exact_mode=True), oracle_advect(oracle, c, NAMES, dt, nsteps=2), f"nz={nz}")
    sweep(run, range(3, HEIGHTS.stop))


def test_every_column_height_fused_donor_cell_pass(oracle, probe):
    """The field after the fused kernel's own donor-cell pass (its output with the antidiffusive coefficients zeroed,
    tests/support/mpdata_probe.hip) bit-identical to the reference's donor-cell pass at every height: the level slots, the
    exchange of the edge levels between waves and level ranges, the ground and the column top."""
    def run(nz):
        c = column_case(oracle, nz)
        dt = ideal.cfl_dt(c)
        check_bits(fused_donor_cell_pass(probe, c, NAMES, dt, fct=nz >= 3), oracle_advect(oracle, c, NAMES, dt, order=1), f"nz={nz} q2")
    sweep(run)


def test_every_column_height_third_order_with_density(oracle):
    """mpdata_order 3 with advect_density: the second launch of each step is the kernel without a donor-cell pass (no q2 exchange
    between waves), and the denominators carry rho"""
    def run(nz):
        c = column_case(oracle, nz)
        fct = nz >= 3
        dt = ideal.cfl_dt(c)
        ref = oracle_advect(oracle, c, NAMES, dt, dens=True, order=3, fct=fct)
        check_close(device_advect(c, NAMES, dt, dens=True, order=3, fct=fct), ref, f"nz={nz}")
    sweep(run)


def test_config4_80_levels_full_size(oracle):
    """configs[4]'s grid, 512 x 512 x 80, the 9 scalars Thompson advects, one step on the ideal hill: the fused kernel (three level
    ranges with halo levels, a wave above the top of the column in the last one) every cell within the gate and its margin, the exact
    mode every cell bit for bit, both against one oracle result; the boundary ring bit for bit."""
    c = ideal.make_case(512, 512, 80, hill_height=1000.0, noise=0.01, n_hydro=1)
    dt = ideal.cfl_dt(c)
    ref = oracle_advect(oracle, c, SCALARS, dt)
    got = device_advect(c, SCALARS, dt)
    check_close(got, ref, "512x512x80 fused", record="512x512x80")
    for n in SCALARS:
        assert bits_equal(got[n][0], ref[n][0]) and bits_equal(got[n][-1], ref[n][-1]), n
        assert bits_equal(got[n][:, :, 0], ref[n][:, :, 0]) and bits_equal(got[n][:, :, -1], ref[n][:, :, -1]), n
    del got
    check_bits(device_advect(c, SCALARS, dt, exact_mode=True), ref, "512x512x80 exact mode")


@pytest.mark.parametrize("dens", [False, True])
def test_config4_80_levels_tile_rough_winds(oracle, dens):
    """configs[4]'s 8-GPU tile, 256 x 128 x 80, the 9 scalars, white noise of 0.5 m/s on u and v (w rebalanced), two steps: the exact
    mode bit for bit; the fused kernel within the gate and its margin at each step, the oracle starting each step from the device's
    state (the gate is a bound per step: the differences of one step are inputs of the next, which the limiter may amplify)"""
    c = roughen_winds(ideal.make_case(256, 128, 80, hill_height=1000.0, noise=0.01, n_hydro=1), oracle, 0.5)
    dt = ideal.cfl_dt(c)
    check_bits(device_advect(c, SCALARS, dt, dens=dens, nsteps=2, exact_mode=True), oracle_advect(oracle, c, SCALARS, dt, dens=dens, nsteps=2),
               f"256x128x80 dens{int(dens)} exact mode")
    state = {n: c[n] for n in SCALARS}
    for step in range(2):
        cs = dict(c); cs.update(state)
        got = device_advect(cs, SCALARS, dt, dens=dens)
        check_close(got, oracle_advect(oracle, cs, SCALARS, dt, dens=dens), f"step {step}", record=f"256x128x80 rough0.5 dens{int(dens)}")
        state = got


# ---- near underflow ----------------------------------------------------------------------------------------------------------
TINY = float(np.finfo(np.float32).tiny)          # FLT_MIN = 2^-126, the smallest normal float
SUB = float(np.finfo(np.float32).smallest_subnormal)   # 2^-149


def underflow_case(oracle, nx=130, ny=40, nz=20, rough=0.5):
    """water_vapor: the ideal qv scaled to at most 64 FLT_MIN -- normal numbers whose fluxes and differences are subnormal, and
    subnormal ones aloft;
    cloud_water: subnormal everywhere (random multiples of 2^-149 up to 2^-127) with empty cells; rain: a 1e-4 blob whose
    surroundings are 1e-39 .. 1e-37 (a cloud edge next to near-underflow air); snow: a few subnormal cells in an otherwise empty field."""
    f32 = np.float32
    c = roughen_winds(ideal.make_case(nx, ny, nz, hill_height=900.0, noise=0.01, n_hydro=1), oracle, rough)
    rng = np.random.default_rng(11)
    qv = c["water_vapor"].astype(np.float64)
    c["water_vapor"] = (qv / qv.max() * 64.0 * TINY).astype(f32)
    sub = rng.integers(0, 1 << 23, (ny, nz, nx)).astype(np.float64) * SUB
    sub[rng.random((ny, nz, nx)) < 0.2] = 0.0
    c["cloud_water"] = sub.astype(f32)
    rain = (10.0 ** rng.uniform(-39, -37, (ny, nz, nx))).astype(f32)
    rain[ny // 2 - 4:ny // 2 + 4, 3:9, nx // 2 - 10:nx // 2 + 10] = f32(1e-4)
    c["rain"] = rain
    snow = np.zeros((ny, nz, nx), f32)
    for (j, k, i) in [(1, 0, 1), (ny // 2, nz // 2, 57), (ny - 2, nz - 1, nx - 2), (ny // 3, 4, 58)]:
        snow[j, k, i] = f32(37 * SUB)
    c["snow"] = snow
    for n in ("water_vapor", "cloud_water", "rain"):
        assert (c[n] > 0).any() and (c[n][c[n] > 0] < TINY).any(), n     # the subnormal range is really in the data
    return c


UNDERFLOW = ["water_vapor", "cloud_water", "rain", "snow"]


def test_near_underflow_upwind_and_exact_mode_bit_exact(oracle):
    """The upwind scheme and MPDATA's exact mode evaluate the reference's operations in its order, and the device keeps subnormal
    floats as the CPU does: every cell of every near-underflow field bit for bit (a flushed subnormal anywhere would be a whole
    cell's value)"""
    c = underflow_case(oracle)
    dt = ideal.cfl_dt(c)
    check_bits(device_advect(c, UNDERFLOW, dt, nsteps=2, scheme=kADV_UPWIND), oracle_advect(oracle, c, UNDERFLOW, dt, nsteps=2, scheme=kADV_UPWIND), "upwind")
    for dens, order in [(False, 2), (True, 3)]:
        ref = oracle_advect(oracle, c, UNDERFLOW, dt, dens=dens, order=order, nsteps=2)
        check_bits(device_advect(c, UNDERFLOW, dt, dens=dens, order=order, nsteps=2, exact_mode=True), ref, f"exact mode dens{int(dens)} order{order}")


def test_near_underflow_fused_donor_cell_pass(oracle, probe):
    """The fused kernel's donor-cell pass (q2) on the near-underflow fields.  Its fluxes are U q rounded once, the reference's
    (2 U q) / 2 rounded twice: the same number while the product is a normal float, not always below FLT_MIN.  There q2 may differ
    by one rounding in each of its two subtractions, so every cell lies within 2 ulp of the reference's q2 plus 8 subnormal steps.
    (q2 is bit-identical wherever the fluxes are normal floats: test_every_column_height_fused_donor_cell_pass.  The limiter's
    all-or-nothing factor next to the ring, which needs that, reaches 1 only for q2 - qmin >= 1e-15 and is ~0 here either way.)"""
    c = underflow_case(oracle)
    dt = ideal.cfl_dt(c)
    got, ref = fused_donor_cell_pass(probe, c, UNDERFLOW, dt), oracle_advect(oracle, c, UNDERFLOW, dt, order=1)
    for n in UNDERFLOW:
        g, r = got[n].astype(np.float64), ref[n].astype(np.float64)
        bound = 2.0 * np.spacing(np.abs(ref[n])).astype(np.float64) + 8 * SUB
        bad = np.abs(g - r) > bound
        assert not bad.any(), f"{n}: {int(bad.sum())} cells beyond 2 ulp + 8 x 2^-149, max |d| = {np.abs(g - r).max() / SUB:.0f} x 2^-149"
        assert (got[n] != c[n]).any(), n


@pytest.mark.parametrize("dens,fct,order", [(False, True, 2), (True, True, 2), (False, False, 2), (False, True, 3)])
def test_near_underflow_fused(oracle, dens, fct, order):
    """The fused kernel on the near-underflow fields, three steps, the oracle each time from the device's state of the step before:
      * every cell within 0.3 of the gate times its local field scale, or within 8 subnormal steps (8 x 2^-149) of the oracle -- a flux
        below FLT_MIN is rounded once there (U q) and twice in the reference ((2 U q) / 2), so a cell whose neighbourhood is itself
        subnormal may differ in its last subnormal bits; a flushed subnormal would miss by the cell's whole value;
      * a cell whose neighbourhood is empty stays exactly zero, and with the limiter no cell turns negative."""
    c = underflow_case(oracle)
    dt = ideal.cfl_dt(c)
    from scipy.ndimage import maximum_filter
    state = {n: c[n].copy() for n in UNDERFLOW}
    for step in range(3):
        cs = dict(c); cs.update(state)
        ref = oracle_advect(oracle, cs, UNDERFLOW, dt, dens=dens, order=order, fct=fct)
        got = device_advect(cs, UNDERFLOW, dt, dens=dens, order=order, fct=fct)
        for n in UNDERFLOW:
            g, r = got[n].astype(np.float64), ref[n].astype(np.float64)
            assert np.isfinite(g).all(), f"step {step} {n}: not finite"
            scale = maximum_filter(np.abs(r), size=5, mode="nearest")
            diff = np.abs(g - r)
            bad = (diff > MPDATA_MARGIN * MPDATA_RTOL * scale) & (diff > 8 * SUB)
            w = np.unravel_index(int(np.argmax(np.where(bad, diff, -1.0))), diff.shape)
            assert not bad.any(), (f"step {step} {n}: {int(bad.sum())} cells beyond both bounds, e.g. {w}: got {g[w]:.6e} oracle {r[w]:.6e} "
                                   f"local scale {scale[w]:.3e}")
            assert np.array_equal(g[scale == 0], r[scale == 0]), f"step {step} {n}: an empty neighbourhood did not stay zero"
            if fct:
                assert g.min() >= 0.0, f"step {step} {n}: min {g.min()!r}"
            assert (got[n] != cs[n]).any(), f"step {step} {n}: advection did nothing"
        state = got

"""The advection where its HORIZONTAL launch layout changes, against the CPU oracle (bit-exact restatement of the compiled reference).
tests/test_gpu_mpdata_columns.py sweeps the column height on one 70 x 10 tile; here the shapes of tests/mpdata_rows_case.py run:
  * widths:  every nx 3 .. 130 and 174 .. 178 -- x tiles that are exactly full, a last tile of one column, the clamped lanes beyond
             the ring, lane_store at every seam; the exact mode's 63-cell tiles at theirs;
  * rows:    every ny 3 .. 70 and the row counts whose last y chunk has 1 .. 6 rows, on one and on two x tiles -- every march of a
             chunk the kernel's schedule can produce (no steady step at all, tails of 0 .. 4 generic steps, a chunk of one row);
  * scalars: 1 .. 11 scalars, fewer work items than XCDs and counts that are no multiple of 8 -- a wrong (tile, chunk, scalar) of a
             block swaps whole fields, and every field has content of its own;
  * ranges:  2 and 3 level ranges together with short last chunks.
At every shape: the upwind scheme, the donor-cell pass inside the fused kernel and the exact mode bit for bit; the fused kernel every
cell within MPDATA_MARGIN x MPDATA_RTOL of the local field scale; the boundary ring of every output bit for bit the input.  On every
fourth shape also the scheme without the limiter, the third order with advect_density, and two calls on one context.
(What the lists rest on -- the layout, the classes they reach, the conditioning of the reference: tests/test_mpdata_rows_inputs.py.)"""
import pytest
from icar_amd import ideal
from icar_amd.options import options_t
from icar_amd.advection import advect
from icar_amd.constants import kADV_UPWIND, kADV_MPDATA
import mpdata_rows_case as R
from test_gpu_mpdata_columns import device_advect, oracle_advect, fused_donor_cell_pass, check_bits, sweep
from util import MEMBER, KVAR, bits_equal, single_image_domain, assert_fields_close, local_rel_err, parity_record

pytestmark = pytest.mark.gpu

# contiguous parts of each list -- and of the shapes of each list that also run the other forms of the scheme (every fourth, the first
# and the last) -- so that no test runs longer than a few seconds
GROUPS = {"widths": 10, "rows": 10, "scalars": 2, "ranges": 3}
VGROUPS = {"widths": 10, "rows": 10, "scalars": 2, "ranges": 3}
PARTS = [(k, g) for k, n in GROUPS.items() for g in range(n)]
VPARTS = [(k, g) for k, n in VGROUPS.items() for g in range(n)]
part = pytest.mark.parametrize("name,g", PARTS, ids=[f"{k}{g}" for k, g in PARTS])
vpart = pytest.mark.parametrize("name,g", VPARTS, ids=[f"{k}{g}" for k, g in VPARTS])


def label(shape):
    return f"{shape[0]}x{shape[1]}x{shape[2]} nv{len(shape[3])}"


def shapes_of(probe, name, g, variants=False):
    """{label: shape} of part g of a list; variants: of the shapes of the list that also run the other forms of the scheme"""
    shapes = R.lists(probe)[name]
    if variants:
        shapes = [shapes[t] for t in R.with_variants(shapes)]
    return {label(s): s for t, s in R.group(shapes, g, (VGROUPS if variants else GROUPS)[name])}


def case_of(oracle, shape):
    c = R.rows_case(oracle, *shape)
    return c, shape[3], ideal.cfl_dt(c)


def check_ring(got, c, what):
    """adv_mpdata.f90:63-65, advect.f90: the boundary ring of the new field is the old one"""
    for n in got:
        assert bits_equal(R.ring(got[n]), R.ring(c[n])), f"{what} {n}: the boundary ring changed"


def check_moved(got, c, what):
    for n in got:
        assert (got[n] != c[n]).any(), f"{what} {n}: advection did nothing"


def check_fused(got, ref, what, worst):
    """every cell within the gate and its margin (no near_gate); worst: the measured maxima, kept for the parity record"""
    for n in ref:
        worst[0] = max(worst[0], local_rel_err(got[n], ref[n])[0])
        assert_fields_close(got[n], ref[n], f"{what} {n}")


def run_sweep(probe, name, g, run, variants=False):
    shapes = shapes_of(probe, name, g, variants)
    sweep(lambda lb: run(shapes[lb], lb), list(shapes), what=f"shapes of {name}/{g}", key="")


@part
def test_upwind_bit_exact(oracle, probe, name, g):
    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        got = device_advect(c, names, dt, scheme=kADV_UPWIND)
        check_bits(got, oracle_advect(oracle, c, names, dt, scheme=kADV_UPWIND), f"{lb} upwind")
        check_ring(got, c, lb); check_moved(got, c, lb)
    run_sweep(probe, name, g, run)
    parity_record("mpdata_rows", f"{name}/{g} upwind", {"all": {"bitdiff_cells": 0}})


@part
def test_fused_donor_cell_pass_bit_exact(oracle, probe, name, g):
    """the fused kernel's own donor-cell pass (its output with the antidiffusive coefficients zeroed), limiter on"""
    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        got = fused_donor_cell_pass(probe, c, names, dt, fct=True)
        check_bits(got, oracle_advect(oracle, c, names, dt, order=1), f"{lb} q2")
        check_ring(got, c, lb); check_moved(got, c, lb)
    run_sweep(probe, name, g, run)
    parity_record("mpdata_rows", f"{name}/{g} fused donor-cell pass", {"all": {"bitdiff_cells": 0}})


@part
def test_exact_mode_bit_exact(oracle, probe, name, g):
    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        got = device_advect(c, names, dt, exact_mode=True)
        check_bits(got, oracle_advect(oracle, c, names, dt), f"{lb} exact mode")
        check_ring(got, c, lb); check_moved(got, c, lb)
    run_sweep(probe, name, g, run)
    parity_record("mpdata_rows", f"{name}/{g} exact mode", {"all": {"bitdiff_cells": 0}})


@part
def test_fused(oracle, probe, name, g):
    """the default path, mpdata_order 2 with the limiter"""
    worst = [0.0]

    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        got = device_advect(c, names, dt)
        check_ring(got, c, lb); check_moved(got, c, lb)
        check_fused(got, oracle_advect(oracle, c, names, dt), lb, worst)
    try:
        run_sweep(probe, name, g, run)
    finally:
        print(f"{name}/{g}: largest deviation of the fused kernel {worst[0]:.3e} of the local field scale")
        parity_record("mpdata_rows", f"{name}/{g} fused", {"all": {"max_over_local_scale": worst[0]}})


def device_two_calls(c, names, dt):
    """two advect calls on one context (the second reads the ping-pong partners the first wrote, with the coefficients of the first
    call's setup): the fields after each"""
    d = single_image_domain(c)
    try:
        opt = options_t(); opt.physics.advection = kADV_MPDATA
        opt.advect_vars([KVAR[n] for n in names])
        out = []
        for _ in range(2):
            advect(d, opt, dt)
            out.append({n: d.get(MEMBER[n]) for n in names})
        return out
    finally:
        d.close()


@vpart
def test_without_limiter_and_third_order_on_every_fourth_shape(oracle, probe, name, g):
    """mpdata_order 2 without the limiter; mpdata_order 3 with advect_density (the second launch of a step is the kernel without a
    donor-cell pass, and the denominators carry rho)"""
    worst = [0.0]

    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        got = device_advect(c, names, dt, fct=False)
        check_ring(got, c, lb)
        check_fused(got, oracle_advect(oracle, c, names, dt, fct=False), f"{lb} no limiter", worst)
        got = device_advect(c, names, dt, dens=True, order=3)
        check_ring(got, c, lb)
        check_fused(got, oracle_advect(oracle, c, names, dt, dens=True, order=3), f"{lb} order 3 with density", worst)
    try:
        run_sweep(probe, name, g, run, variants=True)
    finally:
        parity_record("mpdata_rows", f"{name}/{g} no limiter, order 3 with density", {"all": {"max_over_local_scale": worst[0]}})


@vpart
def test_two_calls_on_one_context_on_every_fourth_shape(oracle, probe, name, g):
    """the fused kernel's second call against the oracle started from the device's state after the first (the gate is a bound per
    step), the exact mode's two calls bit for bit"""
    worst = [0.0]

    def run(shape, lb):
        c, names, dt = case_of(oracle, shape)
        first, second = device_two_calls(c, names, dt)
        check_ring(second, c, lb)
        check_fused(first, oracle_advect(oracle, c, names, dt), f"{lb} first call", worst)
        cs = dict(c); cs.update(first)
        check_fused(second, oracle_advect(oracle, cs, names, dt), f"{lb} second call", worst)
        got = device_advect(c, names, dt, nsteps=2, exact_mode=True)
        check_bits(got, oracle_advect(oracle, c, names, dt, nsteps=2), f"{lb} exact mode, two calls")
        check_ring(got, c, lb)
    try:
        run_sweep(probe, name, g, run, variants=True)
    finally:
        parity_record("mpdata_rows", f"{name}/{g} two calls", {"all": {"max_over_local_scale": worst[0]}})

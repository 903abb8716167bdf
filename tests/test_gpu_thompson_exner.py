"""Thompson computes exner from the pressure in the sub-steps that hide their diagnostics (icar_amd/csrc/timestep.hip:
lazy_diag_part; icar_amd/csrc/mp_thompson.hip: k_thompson_pack_exp, k_thompson_lane_exp).

Inside icar_hip_step / icar_hip_step_n a Thompson sub-step that is not the call's last launches no diagnostic kernel at all; its
interior and strip launches take exner = exner_function(p) instead of loading it.  icar_hip_substep is always its own last
sub-step and loads exner from memory, so:
* step_n(3) == the same three sub-steps as single icar_hip_substep calls, every field the library hands out byte for byte, at
  40 levels (6 columns per block), 56 (512-thread blocks), 60 (one column per wave) and 103 (1024-thread blocks), on tiles whose
  interior width (nx - 2) is no multiple of the columns per block and whose west / east strips are the one-column "tall" form;
* exner overwritten with NaN before step_n(2) and step_n(3) changes nothing: no sub-step that is not the last read it (the first
  one, and the one opened ahead of update_dt); exner after the call is exner_function of the pressure the last sub-step started from;
* the same with a halo of two (the sub-step then issues strips, pack and interior on one stream);
* with rad, pbl, lsm, cu or advect_density on, every sub-step keeps its diagnostic launches, and the results still equal the single
  sub-steps'.
CPU: the new entry points are held to the bounds of the kernels they stand beside (4 waves per SIMD, <= 128 VGPRs, no SGPR spills)."""
import numpy as np
import pytest

import pbl_oracle as P
import ra_oracle as R
from icar_amd import radiation, pbl, surface, convection
from icar_amd import _fields as F
from icar_amd.capi import IcarHipError
from icar_amd.options import options_t
from icar_amd.grid import grid_t
from icar_amd.domain import domain_t
from icar_amd.microphysics import mp_init, mp_var_request
from icar_amd.advection import adv_init
from icar_amd.time_step import substep, step_n, update_dt
from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kRA_SIMPLE, kPBL_SIMPLE, kLSM_BASIC, kWATER_SIMPLE, kCU_BMJ

FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
ANCHOR = (R.GREGORIAN, -(80 * 86400.0 + 30000.0), 365.0, 365.0)
# (nx, ny, nz, uniform dz, dx): a CFL step under the 120 s cap (dx = 2000), so that every sub-step has its own dt; interior widths
# 21 and 11 -- no multiple of 6 (40 levels) or 9 (56, 103 levels) columns per block, nor of the lane kernel's 4 waves per block;
# every tile has more than one row, so its west / east strips are tall
TILES = [(23, 7, 40, None, 2000.0), (23, 7, 56, 220.0, 2000.0), (13, 6, 60, 200.0, 2000.0), (23, 5, 103, 120.0, 2000.0)]
FALLBACK_TILE = (24, 20, 20, None, 5000.0)       # the shape and spacing of the step case of tests/test_gpu_cu_step.py (BMJ finds CAPE)
_cases = {}


def case(oracle, nx, ny, nz, uniform_dz, dx):
    """the step case of tests/test_gpu_cu_step.py at any shape: sheared, noisy winds (every sub-step its own dt once they are
    forced), moist enough for every Thompson species, the surface and radiation inputs, tendencies for the forcing"""
    key = (nx, ny, nz, uniform_dz, dx)
    if key not in _cases:
        c = P.make_case(nx, ny, nz, seed=71, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=dx, water=0.5, uniform_dz=uniform_dz)
        c["water_vapor"] = (c["water_vapor"] * np.float32(1.35)).astype(np.float32)
        rng = np.random.default_rng(71)
        c["u"] = (c["u"] + 6.0 * rng.standard_normal((ny, nz, 1))).astype(np.float32)
        c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, nz, nx))).astype(np.float32)
        c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
        c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
        c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
        c["latitude"] = (np.linspace(-90.0, 90.0, ny)[:, None] + np.zeros((1, nx))).astype(np.float32)
        c["longitude"] = (np.linspace(-180.0, 360.0, nx)[None, :] + rng.uniform(-2, 2, (ny, nx))).clip(-180, 360).astype(np.float32)
        T0 = (c["potential_temperature"] * c["exner"])[:, 0, :]
        c["sst"] = (T0 + rng.uniform(-5, 5, (ny, nx))).astype(np.float32)
        c["skin_temperature"] = (T0 + rng.uniform(-2, 2, (ny, nx))).astype(np.float32)
        c["sensible_heat"] = rng.uniform(-50, 300, (ny, nx)).astype(np.float32)
        c["latent_heat"] = rng.uniform(-20, 200, (ny, nx)).astype(np.float32)
        c["roughness_z0"] = (10.0 ** rng.uniform(-3, -0.5, (ny, nx))).astype(np.float32)
        c["dz_interface"] = c["dz_mass"].copy()
        dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
        dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(np.float32) for k, sc in dq.items()}
        _cases[key] = (c, dq)
    return _cases[key]


def options(c, rad=False, pbl_on=False, lsm=False, cu=False, advect_density=False):
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON
    if rad: opt.physics.radiation = kRA_SIMPLE
    if pbl_on: opt.physics.boundarylayer = kPBL_SIMPLE
    if lsm: opt.physics.landsurface, opt.physics.watersurface = kLSM_BASIC, kWATER_SIMPLE
    if cu: opt.physics.convection = kCU_BMJ
    opt.parameters.advect_density = advect_density
    opt.lsm_options.update_interval = 100
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt); radiation.ra_var_request(opt); pbl.pbl_var_request(opt); surface.lsm_var_request(opt); convection.cu_var_request(opt)
    return opt


def domain(c, dq, opt, halo=None):
    """halo: the grid's halo width (default 1); with a wider one the sub-step issues the strips, the pack and the interior microphysics
    on one stream, a path of its own in icar_substep"""
    if halo is None:
        d = P.device_domain(c)
    else:
        d = domain_t(grid_t().set_grid_dimensions(c["nx"], c["ny"], c["nz"], 1, 1, halo_width=halo), device=0, dx=float(c["dx"]))
        d.load_case(c)
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((c["ny"], c["nx"]), R.SENTINEL, np.float32))
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt); surface.lsm_init(d, opt)
    convection.init_convection(d, opt)
    radiation.rad_calendar(d, *ANCHOR)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def downloads(d):
    """every field the library hands out, as bytes"""
    out = {}
    for n in F.NAMES:
        try:
            out[n] = d.get(n).tobytes()
        except IcarHipError:
            pass
    return out


def assert_same_state(a, b, what):
    x, y = downloads(a), downloads(b)
    assert set(x) == set(y), (what, sorted(set(x) ^ set(y)))
    for n in ("exner", "temperature", "density", "w_real", "accumulated_precipitation", "potential_temperature", "pressure"):
        assert n in x, (what, n)
    bad = [n for n in x if x[n] != y[n]]
    assert not bad, f"{what}: {bad} differ"
    assert a.model_time_seconds == b.model_time_seconds, what


def single_substeps(d, opt, n, before_last=None):
    """n passes of update_dt -> icar_hip_substep -> clock += dt (what icar_hip_step_n runs, one library call per sub-step: each loads
    exner from memory); before_last(d) is called in front of the last one"""
    dts = []
    for m in range(n):
        if m == n - 1 and before_last is not None:
            before_last(d)
        dt = update_dt(d, opt)
        substep(d, opt, dt, forced=FORCED)
        d.model_time_seconds = d.model_time_seconds + dt
        dts.append(dt)
    return dts


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES, ids=lambda t: "x".join(map(str, t[:3])))
def test_step_n_equals_single_substeps(oracle, tile):
    c, dq = case(oracle, *tile)
    opt = options(c)
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    step_n(a, 3, opt, forced=FORCED)
    dts = single_substeps(b, opt, 3)
    assert len(set(dts)) == 3, "every sub-step its own dt wanted"
    assert_same_state(a, b, f"{tile}")
    assert float(a.get("cloud_water_mass").max()) > 1e-6, "the case must have active microphysics"
    a.close(); b.close()


@pytest.mark.gpu
def test_step_n_equals_single_substeps_with_a_halo_of_two(oracle):
    """halo_size 2: the one-stream order of icar_substep (strips -> pack -> interior), which passes the same flag"""
    c, dq = case(oracle, *TILES[0])
    opt = options(c)
    a, b = domain(c, dq, opt, halo=2), domain(c, dq, opt, halo=2)
    a.set("exner", np.full(c["exner"].shape, np.nan, np.float32))
    step_n(a, 3, opt, forced=FORCED)
    single_substeps(b, opt, 3)
    assert_same_state(a, b, "halo 2")
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nsub", [2, 3])
@pytest.mark.parametrize("tile", TILES[:1] + TILES[2:3], ids=lambda t: "x".join(map(str, t[:3])))
def test_hidden_substeps_do_not_read_exner(oracle, tile, nsub):
    c, dq = case(oracle, *tile)
    opt = options(c)
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    a.set("exner", np.full(c["exner"].shape, np.nan, np.float32))
    step_n(a, nsub, opt, forced=FORCED)
    seen = {}

    def keep(d):
        seen.update({k: d.get(k) for k in ("pressure", "potential_temperature", "u", "v", "w")})
    single_substeps(b, opt, nsub, before_last=keep)
    assert_same_state(a, b, f"NaN exner {tile} {nsub}")
    oracle.set_math_mode(0)
    want = oracle.diagnostic_update(seen["pressure"], seen["potential_temperature"], seen["u"], seen["v"], seen["w"], c["dzdx"], c["dzdy"],
                                    c["jacobian"])["exner"]
    assert a.get("exner").tobytes() == want.tobytes(), "exner after the call is exner_function(p) of the last sub-step"
    a.close(); b.close()


FALLBACKS = {"rad": dict(rad=True), "pbl": dict(pbl_on=True), "lsm": dict(lsm=True), "cu": dict(cu=True), "advect_density": dict(advect_density=True)}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(FALLBACKS))
def test_configurations_that_keep_the_diagnostic_launch(oracle, config):
    c, dq = case(oracle, *FALLBACK_TILE)
    opt = options(c, **FALLBACKS[config])
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    step_n(a, 3, opt, forced=FORCED)
    single_substeps(b, opt, 3)
    assert_same_state(a, b, config)
    a.close(); b.close()


def test_exner_from_pressure_entry_points_resources():
    from icar_amd import build as B
    res = B.kernel_resources("mp_thompson.hip")
    for n in ("k_thompson_pack_exp<512>", "k_thompson_pack_exp<1024>", "k_thompson_lane_exp"):
        r = res[n]
        assert r["SGPRs Spill"] == 0, (n, r)
        assert r["Occupancy [waves/SIMD]"] == 4 and r["VGPRs"] <= 128, (n, r)
    for n in ("k_thompson_pack_exp<512>", "k_thompson_pack_exp<1024>"):                 # (the spill bounds of tests/test_kernel_resources.py)
        assert res[n]["VGPRs Spill"] <= 40 and res[n]["ScratchSize [bytes/lane]"] <= 160, (n, res[n])

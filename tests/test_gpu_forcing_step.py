"""The forcing step inside a run (icar_amd/csrc/forcing.hip feeding icar_amd/csrc/timestep.hip), on the device against the CPU:
* two forcing intervals of a whole run at 40 x 12 x 24 (nx x nz x ny): get_initial_conditions (interpolate_forcing without update, the
  first update_winds), then twice [forcing_step with new low-resolution arrays -> icar_hip_step to the next forcing time], against the
  same chain assembled on the CPU from the restatement (tests/forcing_oracle.py) and the step oracle's operators (oracle/orc.py).
  Chosen and held fixed: no microphysics (options%physics%microphysics = 0), MPDATA of water_vapor and potential_temperature in its exact
  mode (icar_hip_mpdata_exact), windtype 0 (make_winds_grid_relative on an unrotated grid + balance_uvw), qv and theta forced on the
  boundaries, u, v, w and the pressure everywhere; a forcing interval of 900 s.  Every forced field, w, exner and density, the count of
  sub-steps of each interval: bit for bit.  Nothing of the model state is uploaded between the two intervals;
* a 2 x 2 tiling of the u / v branch: every tile smooths its own extended grid.  The device gives, bit for bit in every cell of every
  tile's memory, what the restatement gives for that tiling.  Against the one-image result: a tile's extended grid holds the whole
  window of every owned cell, yet a tile is NOT bit-identical to the one-image run, in the reference either: smooth_array starts its
  REAL(8) running row sums from `inputwind(:,j,1) * (windowsize+2)`, a REAL(4) product, and subtracts that row windowsize+1 times in
  REAL(8), so the product's rounding (half a unit in the last place of (windowsize+2) |first row|, nothing when windowsize+2 is a
  power of two) stays in the sums of every later row.  A tile's first row is another one.  Owned cells therefore differ by at most
  2 (windowsize+2)/(2 windowsize+1) 2^-24 max|input| (the two residues, each averaged over the window's rows) plus one unit in the last
  place for the final rounding: asserted, with max|input| taken from the forcing array (the interpolation weights are convex);
* a context that has uploaded forcing data but never called forcing_configure runs sub-steps byte for byte like one that never heard of
  the forcing, refuses interpolate_forcing, and is destroyed cleanly."""
import ctypes

import numpy as np
import pytest

import forcing_oracle as FO
from icar_amd import forcing as F
from icar_amd import ideal
from icar_amd.advection import adv_init, advect
from icar_amd.capi import lib, check, IcarHipError
from icar_amd.constants import kADV_MPDATA, kMP_SB04
from icar_amd.microphysics import mp, mp_init, mp_var_request
from icar_amd.options import options_t
from icar_amd.time_step import step
from icar_amd.wind import update_winds
from util import single_image_domain, bits_equal, nbitdiff

pytestmark = pytest.mark.gpu
f32 = np.float32
NX, NZ, NY = 40, 12, 24
INTERVAL = 900.0
ADV = ["water_vapor", "potential_temperature"]
FORCED = [("water_vapor", True), ("potential_temperature", True), ("pressure", False), ("u", False), ("v", False), ("w", False)]


def test_two_forcing_intervals_of_a_run_equal_the_cpu_chain(oracle):
    c = ideal.make_case(NX, NY, NZ, hill_height=700.0, noise=0.01)
    rng = np.random.default_rng(21)
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(f32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(f32)
    dx = float(c["dx"])
    fc = FO.random_case(31, nx=NX, nz=NZ, ny=NY, nxf=7, nzf=14, nyf=6, nsmooth=2, ext=(2, 2, 2, 2))
    los = [fc["lo1"], fc["lo2"], FO.random_case(32, nx=NX, nz=NZ, ny=NY, nxf=7, nzf=14, nyf=6)["lo1"]]
    for lo in los:                                            # moderate winds: the sub-step count stays in the tens
        lo["u"] *= f32(0.3); lo["v"] *= f32(0.3)
    names = FO.forced_of(fc)
    assert names == FO.FORCED
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = 0; opt.physics.windtype = 0
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = dx; opt.parameters.ideal = True
    opt.advect_vars(ADV)
    sin0, cos1 = np.zeros((NY, NX)), np.ones((NY, NX))
    # ---- the device: nothing but the small forcing arrays goes up after load_case ----
    d = single_image_domain(c)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    adv_init(d, opt)
    d.set("sintheta", sin0); d.set("costheta", cos1)
    F.forcing_configure(d, FO.boundary_of(fc, los[0]), fc["nsmooth"], domain_z=fc["z"])
    d.interpolate_forcing(FO.boundary_of(fc, los[0]), update=False)
    update_winds(d, opt)                                      # the first call of a run: on u, v, w themselves
    n_dev = []
    for k in (1, 2):
        F.forcing_step(d, FO.boundary_of(fc, los[k]), opt, INTERVAL)
        n_dev.append(step(d, k * INTERVAL, opt, forced=FORCED, diagnostics=True))
    # ---- the same chain on the CPU ----
    oracle.set_math_mode(0)
    geom = [c[k] for k in ("jacobian_u", "jacobian_v", "jacobian_w", "advection_dz")]
    s = {}
    FO.interpolate_forcing(fc, {n: los[0][n].copy() for n in names}, s)
    oracle.make_winds_grid_relative(s["u"], s["v"], sin0, cos1)
    s["w"] = oracle.balance_uvw(s["u"], s["v"], *geom, dx)
    t, n_cpu, diag = 0.0, [], None
    for k in (1, 2):
        dq = {}
        FO.interpolate_forcing(fc, {n: los[k][n].copy() for n in names}, dq)
        oracle.make_winds_grid_relative(dq["u"], dq["v"], sin0, cos1)
        dq["w"] = oracle.balance_uvw(dq["u"], dq["v"], *geom, dx)
        FO.update_delta(dq, s, INTERVAL)
        end, n = k * INTERVAL, 0
        while t < end:
            dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], dx))), 120.0)
            if t + dt > end: dt = end - t
            enforce = (end - t) < dt * 2
            diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
            q = np.stack([s[m] for m in ADV]).copy()
            oracle.advect(2, q, s["u"], s["v"], s["w"], diag["density"], c["jacobian"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"],
                          c["advection_dz"], c["dz_levels"], dx, float(f32(dt)))
            for m, name in enumerate(ADV): s[name] = q[m].copy()
            for name, fb in FORCED:
                oracle.apply_forcing(s[name], dq[name], dt, int(fb), 1, 1, 1, 1)
            if enforce:
                for name in ADV: oracle.enforce_limits(s[name])
            t += dt; n += 1
        n_cpu.append(n)
        assert all(np.isfinite(a).all() for a in s.values()), "the case must stay finite"
    assert n_dev == n_cpu and min(n_cpu) >= 6, (n_dev, n_cpu)
    print("sub-steps of the two forcing intervals:", n_cpu)
    for name, _ in FORCED:
        got = d.get(name)
        assert bits_equal(got, s[name]), f"{name}: {nbitdiff(got, s[name])} of {got.size} cells differ after {sum(n_cpu)} sub-steps"
    assert bits_equal(d.get("exner"), diag["exner"]) and bits_equal(d.get("density"), diag["density"])
    # the second interval worked on the rates the second forcing_step left
    for name in names + ["w"]:
        assert bits_equal(d.get_dqdt(name), dq[name]), name
    d.close()


# ---- the 2 x 2 tiling ---------------------------------------------------------------------------------------------------------------
def _tile_case(g, lo, box, ns, nxg, nyg):
    """the tables of one tile cut out of the one-image tables: box = (i_a, i_b, j_a, j_b), the tile's memory in 0-based mass cells of
    the domain, upper ends exclusive; the extended staggered grids reach nsmooth cells further, clipped at the domain's edge"""
    i_a, i_b, j_a, j_b = box
    cut = lambda G, ia, ib, ja, jb: {k: np.ascontiguousarray(G[k][ja:jb, ia:ib] if k in ("x", "y", "w") else G[k][ja:jb, :, ia:ib]) for k in FO.LUT_KEYS}
    c = {"nsmooth": ns, "adjust": False, "geo_z": None, "lo1": lo, "z": np.zeros((j_b - j_a, g["geo"]["z"].shape[1], i_b - i_a), f32)}
    c["geo"] = dict(cut(g["geo"], i_a, i_b, j_a, j_b), i0=0, j0=0)
    ua, ub, va, vb = max(0, i_a - ns), min(nxg + 1, i_b + 1 + ns), max(0, j_a - ns), min(nyg, j_b + ns)
    c["geo_u"] = dict(cut(g["geo_u"], ua, ub, va, vb), i0=i_a - ua, j0=j_a - va)
    ua, ub, va, vb = max(0, i_a - ns), min(nxg, i_b + ns), max(0, j_a - ns), min(nyg + 1, j_b + 1 + ns)
    c["geo_v"] = dict(cut(g["geo_v"], ua, ub, va, vb), i0=i_a - ua, j0=j_a - va)
    return c


@pytest.mark.parametrize("ns", [1, 2])
def test_two_by_two_tiling_of_the_wind_smoothing(ns):
    nxg, nyg, nz, halo = 22, 17, 5, 1
    g = FO.random_case(50 + ns, nx=nxg, nz=nz, ny=nyg, nxf=5, nzf=6, nyf=4, nsmooth=ns, ext=(0, 0, 0, 0))     # one image: the grids end at the domain's edge
    one = {}
    FO.interpolate_forcing(g, {n: g["lo1"][n].copy() for n in ("u", "v")}, one, fields=["u", "v"])
    xs, ys = (0, 11, nxg), (0, 9, nyg)
    for tj in range(2):
        for ti in range(2):
            own = (xs[ti], xs[ti + 1], ys[tj], ys[tj + 1])                                    # owned mass cells
            box = (max(0, own[0] - halo), min(nxg, own[1] + halo), max(0, own[2] - halo), min(nyg, own[3] + halo))
            c = _tile_case(g, g["lo1"], box, ns, nxg, nyg)
            want = {}
            FO.interpolate_forcing(c, {n: g["lo1"][n].copy() for n in ("u", "v")}, want, fields=["u", "v"])
            d = FO.device_domain(c)
            d.interpolate_forcing(FO.boundary_of(c, g["lo1"], ["u", "v"]), update=False)
            got = {n: d.get(n) for n in ("u", "v")}
            d.close()
            for n in ("u", "v"):
                assert FO.bitdiff(got[n], want[n]) == 0, (ti, tj, n, FO.bitdiff(got[n], want[n]))      # the tiling's restatement, every cell of the memory
                # owned cells (u: the owned cells' faces, v likewise) against the one-image result
                oi = slice(own[0] - box[0], own[1] - box[0] + (n == "u")); oj = slice(own[2] - box[2], own[3] - box[2] + (n == "v"))
                a = got[n][oj, :, oi]
                b = one[n][own[2]:own[3] + (n == "v"), :, own[0]:own[1] + (n == "u")]
                assert a.shape == b.shape
                tol = 2.0 * (ns + 2) / (2 * ns + 1) * 2.0 ** -24 * float(np.abs(g["lo1"][n]).max()) + np.spacing(np.maximum(np.abs(a), np.abs(b)))
                assert (np.abs(a.astype(np.float64) - b) <= tol).all(), (ti, tj, n, float(np.abs(a - b).max()))


# ---- a context without forcing_configure ---------------------------------------------------------------------------------------------
def test_a_context_that_never_configured_the_forcing_is_unchanged():
    c = ideal.make_case(NX, NY, NZ, hill_height=700.0, noise=0.01)
    c["water_vapor"] = (c["water_vapor"] * f32(1.5)).astype(f32)
    dt = min(ideal.cfl_dt(c), 40.0)
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_SB04
    mp_var_request(opt)
    members = ["water_vapor", "cloud_water_mass", "rain_mass", "snow_mass", "potential_temperature", "u", "v", "w", "pressure"]
    out = []
    for touched in (False, True):
        d = single_image_domain(c)
        mp_init(opt, d)
        if touched:
            F.forcing_upload(d, "water_vapor", np.ones((4, 5, 6), f32))
            F.forcing_upload(d, "u", np.ones((4, 5, 6), f32))
        for _ in range(3):
            mp(d, opt, dt); d.model_time_seconds += dt
            advect(d, opt, dt)
        if touched:
            ids = (ctypes.c_int * 1)(d.fid("water_vapor"))
            with pytest.raises(IcarHipError, match="icar_hip_forcing_configure has not been called"):
                check(lib().icar_hip_interpolate_forcing(d.ctx, ids, 1, -1, -1, 0), "interpolate_forcing")
            assert bits_equal(F.forcing_download(d, "u", (4, 5, 6)), np.ones((4, 5, 6), f32))
        out.append({n: d.get(n) for n in members} | {"precipitation": d.get("accumulated_precipitation")})
        d.close()                                              # frees the forcing's arrays of a context that uploaded and never configured
    for n in out[0]:
        assert out[0][n].tobytes() == out[1][n].tobytes(), n
    assert not bits_equal(out[0]["water_vapor"], c["water_vapor"]), "the sub-steps must have done something"


def test_forcing_step_refuses_before_the_first_launch():
    """what update_winds or update_delta_fields would refuse, forcing_step refuses before it has made a single rate"""
    c, _ = FO.load_case(sorted(FO.CASES)[2])
    names = FO.forced_of(c)
    opt = options_t(); opt.physics.windtype = 0
    d = FO.device_domain(c)
    d.interpolate_forcing(FO.boundary_of(c, c["lo1"]), update=False)
    with pytest.raises(IcarHipError, match="update_delta_fields needs field 13"):          # w was never uploaded
        F.forcing_step(d, FO.boundary_of(c, c["lo2"]), opt, INTERVAL)
    for n in names:
        with pytest.raises(IcarHipError, match="no dqdt mirror"):
            d.get_dqdt(n)
    d.set("w", c["w"])
    with pytest.raises(IcarHipError, match="update_winds works on the dqdt_3d of u and v"):
        F.forcing_step(d, FO.boundary_of(c, c["lo2"], ["water_vapor"]), opt, INTERVAL)
    with pytest.raises(IcarHipError, match="no dqdt mirror"):
        d.get_dqdt("water_vapor")
    with pytest.raises(IcarHipError, match="positive number of seconds"):
        F.forcing_step(d, FO.boundary_of(c, c["lo2"]), opt, 0.0)
    d.close()

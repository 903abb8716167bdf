"""The Noah branch of lsm() in the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:491) at 24 x 10 x 8 with ra_simple + Noah +
pbl_simple + Thompson + MPDATA (exact mode) on and forced winds; the update gate opens on the first sub-step, stays shut and opens again,
and ICAR_F_PRECIPITATION is raised by the test between two icar_hip_step calls:
* icar_hip_step == the same slots called one by one through the public entry points on a second context, byte for byte;
* icar_hip_step == the loop assembled call by call on the CPU from the oracle's operators and the restatements (ra, sfc, Noah and its
  driver, pbl), every prognostic field, every surface field and every Noah / lsm array bit for bit."""
import numpy as np
import pytest

import lsm_noah_driver_oracle as LN
import noah_oracle as N
import pbl_oracle as P
import ra_oracle as R
import sfc_oracle as S
from icar_amd import radiation, pbl, surface
from icar_amd.options import options_t
from icar_amd.microphysics import mp, mp_init, mp_var_request
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import step
from icar_amd.capi import lib, check
from icar_amd.constants import kADV_MPDATA, kMP_THOMPSON, kRA_SIMPLE, kPBL_SIMPLE, kLSM_NOAH
from util import bits_equal, nbitdiff, parity_record, MEMBER

pytestmark = pytest.mark.gpu
f32 = np.float32
ADV_ORDER = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
OUTPUTS = [MEMBER[n] for n in ADV_ORDER] + ["u", "v", "w", "pressure", "exner", "density", "temperature", "u_mass", "v_mass", "w_real",
                                             "pressure_interface", "accumulated_precipitation"]
NX, NY, NZ = 24, 10, 8
ANCHOR = (R.GREGORIAN, -(80 * 86400.0 + 30000.0), 365.0, 365.0)
RAISE = 2.625                                                               # mm added to the accumulated precipitation between the two steps
NOAH_KEYS = N.OUT + LN.DRV + ["z_atm", "snoalb"]


def step_case(oracle, tab, seed):
    c = P.make_case(NX, NY, NZ, seed=seed, rough=0.0, dt=0.0, th_noise=0.5, hill=900.0, dx=5000.0, water=0.0)
    c["water_vapor"] = (c["water_vapor"] * f32(1.35)).astype(f32)
    rng = np.random.default_rng(seed)
    c["u"] = (c["u"] + 6.0 * rng.standard_normal((NY, NZ, 1))).astype(f32)
    c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, NZ, NX))).astype(f32)
    c["w"] = oracle.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(f32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(f32)
    c["latitude"] = (np.linspace(-60.0, 60.0, NY)[:, None] + np.zeros((1, NX))).astype(f32)
    c["longitude"] = (np.linspace(-180.0, 360.0, NX)[None, :] + rng.uniform(-2, 2, (NY, NX))).clip(-180, 360).astype(f32)
    T0 = (c["potential_temperature"] * c["exner"])[:, 0, :]
    tm = float(T0.mean())
    nc = N.make_case(tab, nx=NX, ny=NY, seed=seed, dt=600.0, t=[tm], sw=[300], pr=[[0.5, 2.0]], snow0=0.3, soil_t=tm - 1.0)
    c["land_mask"] = nc["xland"].astype(np.int32)
    c["skin_temperature"] = (T0 + rng.uniform(-2, 2, (NY, NX))).astype(f32)
    c["sensible_heat"] = rng.uniform(-50, 300, (NY, NX)).astype(f32)
    c["latent_heat"] = rng.uniform(-20, 200, (NY, NX)).astype(f32)
    c["roughness_z0"] = nc["z00"].copy()
    c["dz_interface"] = c["dz_mass"].copy()
    dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
    dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(f32) for k, sc in dq.items()}
    return c, dq, nc


def options(c, update_interval):
    opt = options_t(); opt.physics.advection = kADV_MPDATA; opt.physics.microphysics = kMP_THOMPSON
    opt.physics.radiation, opt.physics.boundarylayer = kRA_SIMPLE, kPBL_SIMPLE
    opt.physics.landsurface, opt.physics.watersurface = kLSM_NOAH, 0
    opt.lsm_options.update_interval = update_interval
    opt.lsm_options.max_swe = 25.0
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt); radiation.ra_var_request(opt); pbl.pbl_var_request(opt); surface.lsm_var_request(opt)
    return opt


def noah_state(c, nc):
    """N.state0 of the Noah case with the step case's surface fields in it"""
    A = LN.state0(nc)
    for k, m in (("tsk", "skin_temperature"), ("hfx", "sensible_heat"), ("lh", "latent_heat"), ("znt", "roughness_z0")):
        A[k] = c[m].copy()
    A["qsfc"] = c["water_vapor"][:, 0, :].copy()                              # lsm_driver.f90:568
    return A


def domain(tab, c, dq, nc, opt):
    d = P.device_domain(c)
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((NY, NX), R.SENTINEL, f32))
    d._noah_win = None
    surface.noah_tables(d, tab)
    A = noah_state(c, nc)
    for k in ("ivgtyp", "isltyp", "vegfra", "tmn"):
        N.device_set(d, k, nc[k])
    N.device_set(d, "smois", nc["smois0"]); N.device_set(d, "tslb", nc["tslb0"])
    for k in ("albedo", "snow", "snowh", "canwat", "lai", "z0", "qsfc", "qfx"):
        N.device_set(d, k, A[k])
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt)
    surface.noah_init(d, opt, fndsnowh=False)
    radiation.rad_calendar(d, *ANCHOR)
    d.configure(opt, forced=FORCED, diagnostics=True)
    d.diagnostic_update(3)                                                    # temperature, surface_pressure, the 10 m winds: lsm_init reads them
    surface.noah_couple(d)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def day_of_year(t):
    cal, start, yd, nyd = ANCHOR
    D = (t - start) / 86400.0
    return (D - yd, nyd) if D >= yd else (D, yd)


def noah_arrays(d):
    return {k: LN.device_get(d, k) for k in NOAH_KEYS}


def test_step_equals_the_slots_one_by_one_and_the_cpu_chain(th_oracle, oracle):
    tab = N.load_tables()
    nx, ny, nz = NX, NY, NZ
    c, dq, nc = step_case(oracle, tab, seed=61)
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    ui = max(int(2.5 * dt0), 1)
    opt = options(c, ui)
    ends = (3.2 * dt0, 6.4 * dt0)
    # ---- the device: two icar_hip_step calls, the precipitation raised in between
    d = domain(tab, c, dq, nc, opt)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    n_dev = step(d, ends[0], opt, forced=FORCED, diagnostics=True)
    d.set("accumulated_precipitation", d.get("accumulated_precipitation") + RAISE)
    n_dev += step(d, ends[1], opt, forced=FORCED, diagnostics=True)
    # ---- a second context: the same slots through the public entry points, with the dt the CPU chain finds
    b = domain(tab, c, dq, nc, opt)
    check(lib().icar_hip_mpdata_exact(b.ctx, 1), "mpdata_exact")
    # ---- the CPU chain
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
    A = noah_state(c, nc)
    N.lsm_init(tab, nc, A)
    sfc = dict(roughness_z0=A["znt"], skin_temperature=A["tsk"], sensible_heat=A["hfx"], latent_heat=A["lh"], qsfc=A["qsfc"], qfx=A["qfx"],
               u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32))
    par = dict(sfc_layer_thickness=400.0, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0, kts=1)
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    mask = np.ascontiguousarray(c["land_mask"], f32)
    drv = dict(nx=nx, ny=ny, xland=mask, terrain=c["terrain"], z1=np.ascontiguousarray(c["z"][:, 0, :]), max_swe=f32(25.0), update_interval=ui,
               precip0=acc)
    noah_static = {k: nc[k] for k in ("nx", "ny", "ivgtyp", "isltyp", "vegfra", "tmn", "shdmin", "shdmax", "fndsnowh")}
    noah_static["xland"] = mask
    diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
    drv["forcing"] = [dict(t=np.ascontiguousarray(diag["temperature"][:, 0, :]), qv=np.ascontiguousarray(s["water_vapor"][:, 0, :]))]
    L = LN.lib()
    import ctypes
    ci, p_ = ctypes.c_int, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    F0 = drv["forcing"][0]
    L.lnd_oracle_couple(ci(nx), ci(ny), p_(A["znt"]), p_(drv["z1"]), p_(drv["terrain"]), p_(F0["t"]), p_(F0["qv"]), p_(acc), p_(A["z0"]), p_(A["chs"]),
                        p_(A["chs2"]), p_(A["rainbl_step"]), p_(A["rainbl8"]), p_(A["t2"]), p_(A["q2"]), p_(A["z_atm"]), p_(A["lnz"]), p_(A["base"]))
    t, n_cpu, t_mp, gates = 0.0, 0, None, []
    for end in ends:
        while t < end:                                                                                      # time_step.f90:462
            dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
            if t + dt > end: dt = end - t
            enforce = (end - t) < dt * 2
            dt4 = float(f32(dt))
            # the second context, slot by slot
            b.diagnostic_update(3)                                                                          # :474
            radiation.rad(b, opt, dt)                                                                       # :488
            surface.lsm(b, opt, dt)                                                                         # :491
            pbl.pbl(b, opt, dt)                                                                             # :494
            mp(b, opt, dt, halo=1); b.halo_send(); mp(b, opt, dt, subset=1); b.halo_retrieve()              # :512-526
            advect(b, opt, dt)                                                                              # :529
            b.apply_forcing(dt, FORCED)                                                                     # :534
            if enforce: b.enforce_limits([MEMBER[n] for n in ADV_ORDER])
            b.model_time_seconds += dt
            # the CPU
            diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
            cc = dict(par, density=diag["density"], exner=diag["exner"], temperature=diag["temperature"], u_mass=diag["u_mass"], v_mass=diag["v_mass"],
                      z=c["z"], terrain=c["terrain"], dz_interface=c["dz_interface"])
            Af = dict(sfc, potential_temperature=s["potential_temperature"], water_vapor=s["water_vapor"])
            S.diag_10m(cc, Af)
            if dt > 1e-3:
                D, yd = day_of_year(t)
                Ar = dict(rad2d); Ar["potential_temperature"] = s["potential_temperature"]
                inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
                R.ra_simple(Ar, inputs, D, yd, ANCHOR[0], dt4, 2, nx - 1, 2, ny - 1, 1, nz)
                is_open, lsm_dt = LN.gate(drv, A, t)
                gates.append(is_open)
                if is_open:
                    lvl = lambda a, k: np.ascontiguousarray(a[:, k, :])
                    F = dict(qv=lvl(s["water_vapor"], 0), t=lvl(diag["temperature"], 0), p8w1=lvl(diag["pressure_interface"], 0),
                             p8w2=lvl(diag["pressure_interface"], 1), swdown=rad2d["shortwave"], glw=rad2d["longwave"], u10=sfc["u_10m"], v10=sfc["v_10m"],
                             psfc=diag["surface_pressure"], precip=acc)
                    drv["forcing"] = [F]
                    LN.pre(drv, A, 0)
                    N.lsm_noah(tab, dict(noah_static, forcing=[F]), A, 0, (2, nx - 1, 2, ny - 1), lsm_dt)
                    LN.post(drv, A, 0, (2, nx - 1, 2, ny - 1))
                S.apply_fluxes(cc, Af, dt4)
                P.simple_pbl({k: s[k] for k in P.SCALARS}, diag["u_mass"], diag["v_mass"], diag["exner"], diag["density"], c["z"], c["dz_mass"],
                             c["terrain"], c["land_mask"], 2, nx - 1, 2, ny - 1, 1, nz, dt4)
            z = [np.zeros((ny, nx), f32) for _ in range(5)]
            mp_dt = dt4 if t_mp is None else float(f32(t - t_mp)); t_mp = t
            th_oracle.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"],
                               s["rain_number"], s["potential_temperature"], diag["exner"], s["pressure"], c["dz_mass"], mp_dt, *z,
                               1, nx, 1, ny, 1, nz, 2, nx - 1, 2, ny - 1, 1, nz)
            acc += z[0]
            q = np.stack([s[n] for n in ADV_ORDER]).copy()
            oracle.advect(2, q, s["u"], s["v"], s["w"], diag["density"], c["jacobian"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"],
                          c["advection_dz"], c["dz_levels"], float(c["dx"]), dt4)
            for m, n in enumerate(ADV_ORDER): s[n] = q[m].copy()
            for n, fb in FORCED:
                oracle.apply_forcing(s[n], dq[n], dt, int(fb), 1, 1, 1, 1)
            if enforce:
                for n in ADV_ORDER: oracle.enforce_limits(s[n])
            t += dt; n_cpu += 1
        if end == ends[0]:
            acc += RAISE
            b.set("accumulated_precipitation", b.get("accumulated_precipitation") + RAISE)
    assert n_dev == n_cpu and n_cpu >= 6, (n_dev, n_cpu)
    assert gates[0] and False in gates and True in gates[gates.index(False):], f"the gate: open, shut, open again: {gates}"
    # the step against the slots one by one: byte for byte
    for m in OUTPUTS + R.OUTPUTS[1:] + S.STATE2:
        assert d.get(m).tobytes() == b.get(m).tobytes(), f"icar_hip_step differs from the slots one by one in {m}"
    got, one = noah_arrays(d), noah_arrays(b)
    for k in NOAH_KEYS:
        assert got[k].tobytes() == one[k].tobytes(), f"icar_hip_step differs from the slots one by one in {k}"
    # the step against the CPU chain
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        g = d.get(dev_name[n])
        assert bits_equal(g, s[n]), f"{n}: {nbitdiff(g, s[n])} of {g.size} cells differ after {n_cpu} sub-steps"
    for k in S.STATE2:
        g = d.get(k)
        assert bits_equal(g, sfc[k]), f"{k}: {nbitdiff(g, sfc[k])} of {g.size} cells differ"
    for k in R.OUTPUTS[1:]:
        assert bits_equal(d.get(k), rad2d[k]), k
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    for k in NOAH_KEYS:
        assert LN.bitdiff(got[k], A[k]) == 0, f"{k}: {LN.bitdiff(got[k], A[k])} values differ from the CPU chain"
    assert (A["rainbl_step"] > 2.0).any(), "the raised precipitation reached lsm_noah"
    parity_record("lsm_noah_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps", {k: {"bitdiff_cells": 0} for k in list(s) + NOAH_KEYS})
    for x in (d, b):
        x.close()

"""The 2-D forced variables in the sub-step loop (icar_amd/csrc/forcing2d.hip behind icar_amd/csrc/timestep.hip; time_step.f90:534) at
24 x 10 x 8 with radiation = 0 (prescribed shortwave / longwave), Noah coupled with water_simple (which reads the forced sst), pbl_simple,
Thompson, MPDATA in its exact mode and forced winds; sst, shortwave, longwave and external_precipitation enabled with non-zero rates:
* icar_hip_step (and icar_hip_step_n) == the same slots and icar_hip_apply_forcing_2d called one by one through the public entry points
  on a second context, byte for byte;
* icar_hip_step (and _step_n) == the loop assembled call by call on the CPU from the oracle's operators and the restatements (sfc, Noah
  and its driver, pbl, the 2-D forcing), every prognostic field, every surface field, every Noah / lsm array and the four variables bit
  for bit;
* the same run with nothing enabled gives OTHER sst, shortwave, skin_temperature, sensible_heat and accumulated precipitation (a no-op
  would not pass), and byte for byte what a context gives that never heard of the family."""
import numpy as np
import pytest

import forcing_oracle as FO
import forcing2d_oracle as F2
import lsm_noah_driver_oracle as LN
import noah_oracle as N
import pbl_oracle as P
import sfc_oracle as S
import test_gpu_lsm_noah_step as TN
from icar_amd import forcing as F
from icar_amd import pbl, surface
from icar_amd.advection import advect
from icar_amd.capi import lib, check
from icar_amd.constants import kWATER_SIMPLE
from icar_amd.microphysics import mp
from icar_amd.time_step import step, step_n
from util import bits_equal, nbitdiff, MEMBER

pytestmark = pytest.mark.gpu
f32 = np.float32
NX, NY, NZ = TN.NX, TN.NY, TN.NZ
ADV_ORDER, FORCED = TN.ADV_ORDER, TN.FORCED
INTERVAL = 1800.0                                                            # dt%seconds() of the forcing interval the rates are for
NXF, NYF = 5, 4
OUT2D = ["sst", "shortwave", "longwave"]


@pytest.fixture(scope="module")
def world(oracle):
    tab = N.load_tables()
    c, dq, nc = TN.step_case(oracle, tab, seed=67)
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    opt = TN.options(c, max(int(2.5 * dt0), 1))
    opt.physics.radiation, opt.physics.watersurface = 0, kWATER_SIMPLE
    rng = np.random.default_rng(670)
    G = FO.random_luts(rng, NX, NZ, NY, NXF, 2, NYF)
    lo = [F2.fields(rng, NYF, NXF, s) for s in (0.0, 1.5)]
    data = {v: F2.geo_interp2d(lo[0][v], G) for v in F2.VARS}
    rate = {v: F2.geo_interp2d(lo[1][v], G) for v in F2.VARS}
    for v in F2.VARS:
        F2.delta(rate[v], data[v], INTERVAL)
        assert (rate[v] != 0).mean() > 0.5, v
    assert (c["land_mask"] == 2).sum() >= 5 and (c["land_mask"] == 1).sum() >= 100, "water_simple and Noah both need cells"
    return dict(tab=tab, c=c, dq=dq, nc=nc, opt=opt, dt0=dt0, G=G, lo=lo, data=data, rate=rate)


def domain(w, family):
    """family: "enabled" / "disabled" (everything but icar_hip_forcing2d_enable) / None (the three slots are set by the host)"""
    d = TN.domain(w["tab"], w["c"], w["dq"], w["nc"], w["opt"])
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    if family is None:
        for v in OUT2D:
            d.set(v, w["data"][v])
        return d
    G = w["G"]
    F.forcing_configure(d, F.boundary_t(F.geo_t(*(G[k] for k in FO.LUT_KEYS), forcing_shape=(NYF, 2, NXF))), 1)
    for v in F2.VARS:
        F.forcing2d_upload(d, v, w["lo"][0][v])
    d.interpolate_forcing_2d(F2.VARS, update=False)
    for v in F2.VARS:
        F.forcing2d_upload(d, v, w["lo"][1][v])
    d.interpolate_forcing_2d(F2.VARS, update=True)
    d.update_delta_fields_2d(F2.VARS, INTERVAL)
    if family == "enabled":
        F.forcing2d_enable(d, F2.VARS)
    return d


def outputs(d, family=True):
    out = {m: d.get(m) for m in TN.OUTPUTS + OUT2D + S.STATE2}
    out.update({"noah_" + k: a for k, a in TN.noah_arrays(d).items()})
    if family:
        out["external_precipitation"] = F.forcing2d_get(d, "external_precipitation")
    return out


def run_three_ways(w, oracle, th_oracle, n_steps=None, end=None):
    """the device loop (icar_hip_step to `end`, or icar_hip_step_n over n_steps), the slots one by one on a second context and the CPU
    chain; returns (outputs of the loop, of the slots, the CPU's fields, the number of sub-steps)"""
    c, dq, nc, opt, tab = w["c"], w["dq"], w["nc"], w["opt"], w["tab"]
    nx, ny, nz = NX, NY, NZ
    d = domain(w, "enabled")
    if end is not None:
        n_dev = step(d, end, opt, forced=FORCED, diagnostics=True)
    else:
        step_n(d, n_steps, opt, forced=FORCED, diagnostics=True); n_dev = n_steps
    b = domain(w, "enabled")
    # ---- the CPU chain
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    two = {v: w["data"][v].copy() for v in F2.VARS}
    A = TN.noah_state(c, nc)
    N.lsm_init(tab, nc, A)
    sfc = dict(roughness_z0=A["znt"], skin_temperature=A["tsk"], sensible_heat=A["hfx"], latent_heat=A["lh"], qsfc=A["qsfc"], qfx=A["qfx"],
               u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32))
    par = dict(sfc_layer_thickness=400.0, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0, kts=1)
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    mask = np.ascontiguousarray(c["land_mask"], f32)
    drv = dict(nx=nx, ny=ny, xland=mask, terrain=c["terrain"], z1=np.ascontiguousarray(c["z"][:, 0, :]), max_swe=f32(25.0),
               update_interval=opt.lsm_options.update_interval, precip0=acc)
    noah_static = {k: nc[k] for k in ("nx", "ny", "ivgtyp", "isltyp", "vegfra", "tmn", "shdmin", "shdmax", "fndsnowh")}
    noah_static["xland"] = mask
    diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
    drv["forcing"] = [dict(t=np.ascontiguousarray(diag["temperature"][:, 0, :]), qv=np.ascontiguousarray(s["water_vapor"][:, 0, :]))]
    # (the coupling: LN.lsm_init's second half)
    import ctypes
    ci, p_ = ctypes.c_int, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    F0 = drv["forcing"][0]
    LN.lib().lnd_oracle_couple(ci(nx), ci(ny), p_(A["znt"]), p_(drv["z1"]), p_(drv["terrain"]), p_(F0["t"]), p_(F0["qv"]), p_(acc), p_(A["z0"]), p_(A["chs"]),
                               p_(A["chs2"]), p_(A["rainbl_step"]), p_(A["rainbl8"]), p_(A["t2"]), p_(A["q2"]), p_(A["z_atm"]), p_(A["lnz"]), p_(A["base"]))
    t, n_cpu, t_mp, gates = 0.0, 0, None, []
    while (t < end) if end is not None else (n_cpu < n_steps):                                              # time_step.f90:462
        dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
        if end is not None and t + dt > end: dt = end - t
        enforce = end is not None and (end - t) < dt * 2
        dt4 = float(f32(dt))
        # the second context, slot by slot
        b.diagnostic_update(3)                                                                          # :474
        surface.lsm(b, opt, dt)                                                                         # :491
        pbl.pbl(b, opt, dt)                                                                             # :494
        mp(b, opt, dt, halo=1); b.halo_send(); mp(b, opt, dt, subset=1); b.halo_retrieve()              # :512-526
        advect(b, opt, dt)                                                                              # :529
        b.apply_forcing(dt, FORCED)                                                                     # :534
        b.apply_forcing_2d(dt)                                                                          # :534, the two_d branch and the precipitation sum
        if enforce: b.enforce_limits([MEMBER[n] for n in ADV_ORDER])
        b.model_time_seconds += dt
        # the CPU
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
        cc = dict(par, density=diag["density"], exner=diag["exner"], temperature=diag["temperature"], u_mass=diag["u_mass"], v_mass=diag["v_mass"],
                  surface_pressure=diag["surface_pressure"], sst=two["sst"], land_mask=c["land_mask"], z=c["z"], terrain=c["terrain"],
                  dz_interface=c["dz_interface"])
        Af = dict(sfc, potential_temperature=s["potential_temperature"], water_vapor=s["water_vapor"])
        S.diag_10m(cc, Af)
        if dt > 1e-3:
            is_open, lsm_dt = LN.gate(drv, A, t)
            gates.append(is_open)
            if is_open:
                lvl = lambda a, k: np.ascontiguousarray(a[:, k, :])
                Fn = dict(qv=lvl(s["water_vapor"], 0), t=lvl(diag["temperature"], 0), p8w1=lvl(diag["pressure_interface"], 0),
                          p8w2=lvl(diag["pressure_interface"], 1), swdown=two["shortwave"], glw=two["longwave"], u10=sfc["u_10m"], v10=sfc["v_10m"],
                          psfc=diag["surface_pressure"], precip=acc)
                drv["forcing"] = [Fn]
                LN.pre(drv, A, 0)
                S.water_simple(cc, Af)                                                                  # lsm_driver.f90:1051-1073
                N.lsm_noah(tab, dict(noah_static, forcing=[Fn]), A, 0, (2, nx - 1, 2, ny - 1), lsm_dt)
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
        for v in F2.VARS:                                                                               # domain_obj.f90:2400-2402
            F2.apply(two[v], w["rate"][v], dt)
        F2.precip(acc, two["external_precipitation"], dt)                                               # :2442-2444
        if enforce:
            for n in ADV_ORDER: oracle.enforce_limits(s[n])
        t += dt; n_cpu += 1
    assert n_dev == n_cpu and n_cpu >= 3, (n_dev, n_cpu)
    assert gates[0] and gates.count(True) >= 2, f"the lsm gate opens more than once: {gates}"
    got, one = outputs(d), outputs(b)
    for x in (d, b):
        x.close()
    cpu = dict(s=s, sfc=sfc, two=two, acc=acc, A=A)
    return got, one, cpu, n_cpu


def compare(got, one, cpu, n):
    for m in got:                                                            # the loop against the slots one by one: byte for byte
        assert got[m].tobytes() == one[m].tobytes(), f"the loop differs from the slots one by one in {m}"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for k in ADV_ORDER + ["u", "v", "w", "pressure"]:
        g = got[dev_name[k]]
        assert bits_equal(g, cpu["s"][k]), f"{k}: {nbitdiff(g, cpu['s'][k])} of {g.size} cells differ after {n} sub-steps"
    for k in S.STATE2:
        assert bits_equal(got[k], cpu["sfc"][k]), f"{k}: {nbitdiff(got[k], cpu['sfc'][k])} of {got[k].size} cells differ"
    for v in F2.VARS:
        assert F2.bitdiff(got[v], cpu["two"][v]) == 0, f"{v}: {F2.bitdiff(got[v], cpu['two'][v])} cells differ"
    assert F2.bitdiff(got["accumulated_precipitation"], cpu["acc"]) == 0
    for k in TN.NOAH_KEYS:
        assert LN.bitdiff(got["noah_" + k], cpu["A"][k]) == 0, f"{k}: {LN.bitdiff(got['noah_' + k], cpu['A'][k])} values differ from the CPU chain"


def test_step_equals_the_slots_one_by_one_and_the_cpu_chain(world, oracle, th_oracle):
    got, one, cpu, n = run_three_ways(world, oracle, th_oracle, end=4.3 * world["dt0"])
    compare(got, one, cpu, n)
    # the rates did something: the forced variables are not where the initial interpolation left them
    for v in F2.VARS:
        assert (got[v] != world["data"][v]).mean() > 0.5, v


def test_step_n_equals_the_slots_one_by_one_and_the_cpu_chain(world, oracle, th_oracle):
    got, one, cpu, n = run_three_ways(world, oracle, th_oracle, n_steps=4)
    compare(got, one, cpu, n)


def test_nothing_enabled_is_another_run_and_the_run_of_a_context_without_the_family(world):
    end, opt = 4.3 * world["dt0"], world["opt"]
    res = {}
    for family in ("enabled", "disabled", None):
        d = domain(world, family)
        n = step(d, end, opt, forced=FORCED, diagnostics=True)
        assert n >= 3
        res[family] = outputs(d, family=False)
        d.close()
    for m in ("sst", "shortwave", "skin_temperature", "sensible_heat", "accumulated_precipitation"):
        assert res["enabled"][m].tobytes() != res["disabled"][m].tobytes(), f"{m} is the same with and without the 2-D forcing"
        assert (res["enabled"][m] != res["disabled"][m]).sum() >= 5, m
    for m in res[None]:
        assert res["disabled"][m].tobytes() == res[None][m].tobytes(), f"uploaded and interpolated but never enabled: {m} differs from a context without the family"

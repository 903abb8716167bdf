"""The YSU scheme in the pbl slot of the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:494):
* icar_hip_step over three or more sub-steps with rad + lsm + YSU + BMJ + Thompson + MPDATA (exact mode) on and forced winds == the
  same loop assembled call by call on the CPU from the oracle's operators and the restatements, every prognostic field, every surface
  field and every array of the two column slots bit for bit.  YSU reads domain%temperature, the mass-point winds, the 10 m winds and
  ustar as diagnostic_update left them, not recomputed after rad and lsm changed the potential temperature;
* icar_hip_substep with YSU initialised == the plain sequence issued call by call, the pbl slot one level down (icar_hip_ysu_sfc,
  icar_hip_ysu, the update and the resets done by the host);
* a 2 x 2 tiling equals the single tile in every owned cell (the scheme is column-local on owned columns; da_sfc_wtq and the update
  run over each image's memory, where a halo cell holds what its owner holds);
* a context initialised with pbl_init(ctx, 2) is byte-identical to one configured with pbl_configure(ctx, 2);
* with boundarylayer = 0 a sub-step's outputs are byte-identical to those of a context that never heard of pbl_init, also after YSU
  was initialised and has been switched off;
* smoke() passes with its YSU case."""
import numpy as np
import pytest

import bmj_oracle as B
import pbl_oracle as P
import ra_oracle as R
import sfc_oracle as S
import ysu_oracle as Y
import test_gpu_cu_step as CS
from icar_amd import radiation, pbl, surface, convection
from icar_amd.microphysics import mp_init
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import substep, step
from icar_amd.capi import lib, check
from icar_amd.constants import kPBL_SIMPLE, kPBL_YSU, kWATER_SIMPLE, kLSM_BASIC
from icar_amd.grid import grid_t
from icar_amd.ideal import cut_tile
from util import bits_equal, nbitdiff, parity_record, MEMBER

pytestmark = pytest.mark.gpu
ADV_ORDER, FORCED, OUTPUTS, ANCHOR = CS.ADV_ORDER, CS.FORCED, CS.OUTPUTS, CS.ANCHOR
NX, NY, NZ = 26, 14, 12
YSU_ARRAYS = ["hpbl", "kpbl", "exch_h", "psim", "psih", "regime", "ri", "windspd", "hol"] + Y.TEND
f32 = np.float32


def step_case(oracle, seed):
    CS.NX, CS.NY, CS.NZ = NX, NY, NZ                                          # the convection step case on 26 x 14 x 12
    try:
        c, dq = CS.step_case(oracle, seed)
    finally:
        CS.NX, CS.NY, CS.NZ = 24, 20, 20
    rng = np.random.default_rng(900 + seed)
    c["ground_surf_temperature"] = (c["skin_temperature"] + rng.normal(0, 0.5, (NY, NX))).astype(f32)
    return c, dq


def options(c, bl=kPBL_YSU, others=True):
    opt = CS.options(c, others)
    opt.physics.boundarylayer = bl
    pbl.pbl_var_request(opt)
    return opt


def domain(c, dq, opt):
    d = P.device_domain(c)
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((NY, NX), R.SENTINEL, f32))
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt); surface.lsm_init(d, opt)
    convection.init_convection(d, opt)
    if opt.physics.boundarylayer == kPBL_YSU:
        pbl.ysu_set(d, "ground_surf_temperature", c["ground_surf_temperature"])
    radiation.rad_calendar(d, *ANCHOR)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def ysu_state(c):
    ny, nz, nx = c["z"].shape
    A = Y.init_arrays(c)                                                     # pbl_init, from the roughness of the start
    for k in Y.TEND + ["exch_h"]:
        A[k] = np.zeros((ny, nz, nx), f32)
    for k in ("hpbl", "psim", "psih", "regime", "ri", "windspd"):
        A[k] = np.zeros((ny, nx), f32)
    A["kpbl"] = np.zeros((ny, nx), np.int32)
    return A


def test_whole_step_loop_with_ysu_equals_cpu_chain(th_oracle, oracle):
    nx, ny, nz = NX, NY, NZ
    c, dq = step_case(oracle, seed=71)
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    ui = max(int(1.5 * dt0), 1)
    opt = options(c)
    opt.lsm_options.update_interval = ui
    d = domain(c, dq, opt)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    end = 3.4 * dt0
    n_dev = step(d, end, opt, forced=FORCED, diagnostics=True)
    s = {k: c[k].copy() for k in ADV_ORDER + ["u", "v", "w", "pressure"]}
    rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
    sfc = {k: c[k].copy() for k in ("roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")}
    sfc.update(u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32),
               qsfc=c["water_vapor"][:, 0, :].copy(), qfx=np.zeros((ny, nx), f32), last_model_time=-999.0)
    par = dict(watersurface=kWATER_SIMPLE, landsurface=kLSM_BASIC, sfc_layer_thickness=400.0, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0,
               update_interval=ui, kts=1)
    cu = dict(cldefi=np.full((ny, nx), B.AVGEFI(), f32), tend_th=np.zeros((ny, nz, nx), f32), tend_qv=np.zeros((ny, nz, nx), f32))
    for k in ("raincv", "cutop", "cubot", "accumulated_convective_pcp"):
        cu[k] = np.zeros((ny, nx), f32)
    ys = ysu_state(c)
    acc = np.zeros((ny, nx), np.float64)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, t_mp, moved, mixing = 0.0, 0, None, 0.0, 0
    tile = (2, nx - 1, 2, ny - 1)
    while t < end:                                                                                      # time_step.f90:462
        dt = min(float(f32(0.9) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))), 120.0)
        if t + dt > end: dt = end - t
        enforce = (end - t) < dt * 2
        dt4 = float(f32(dt))
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        cc = dict(par, density=diag["density"], exner=diag["exner"], temperature=diag["temperature"], u_mass=diag["u_mass"], v_mass=diag["v_mass"],
                  surface_pressure=diag["surface_pressure"], z=c["z"], terrain=c["terrain"], sst=c["sst"], land_mask=c["land_mask"], dz_interface=c["dz_interface"])
        A = dict(sfc, potential_temperature=s["potential_temperature"], water_vapor=s["water_vapor"])
        S.diag_10m(cc, A)                                                                               # :143-161
        if dt > 1e-3:                                                                                   # :483
            D, yd = CS.day_of_year(t)                                                                   # :488 rad
            Ar = dict(rad2d); Ar["potential_temperature"] = s["potential_temperature"]
            inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
            R.ra_simple(Ar, inputs, D, yd, ANCHOR[0], dt4, 2, nx - 1, 2, ny - 1, 1, nz)
            if S.gate(cc, A, t): S.water_simple(cc, A)                                                  # :491 lsm
            S.apply_fluxes(cc, A, dt4)
            sfc["last_model_time"] = A["last_model_time"]
            # :494 pbl, kPBL_YSU: what diagnostic_update left (temperature, mass-point and 10 m winds, ustar), the CURRENT scalars and surface fluxes
            moved = max(moved, float(np.abs(s["potential_temperature"] * diag["exner"] - diag["temperature"]).max()))
            yc = dict(z=c["z"], dx=c["dx"], terrain=c["terrain"], land_mask=c["land_mask"], dz_interface=c["dz_interface"],
                      ground_surf_temperature=c["ground_surf_temperature"], pressure=s["pressure"], exner=diag["exner"],
                      pressure_interface=diag["pressure_interface"], surface_pressure=diag["surface_pressure"], u_mass=diag["u_mass"], v_mass=diag["v_mass"])
            yc.update({k: A[k] for k in ("u_10m", "v_10m", "ustar", "roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")})
            yc = {k: (np.ascontiguousarray(v, np.int32 if k == "land_mask" else f32) if isinstance(v, np.ndarray) else v) for k, v in yc.items()}
            YA = dict(ys, temperature=np.ascontiguousarray(diag["temperature"], f32), water_vapor=s["water_vapor"], cloud_water=s["cloud_water"],
                      cloud_ice=s["cloud_ice"], potential_temperature=s["potential_temperature"])
            Y.run_sfc(yc, YA)
            Y.run_ysu(yc, YA, dt4, tile=tile)
            mixing += int((YA["kpbl"] > 1).sum())
            Y.run_apply(yc, YA, dt4)
            ys.update({k: YA[k] for k in ys})
            # :509 convect
            ccu = dict(density=diag["density"], exner=diag["exner"], pressure=s["pressure"], pressure_interface=diag["pressure_interface"],
                       dz_interface=c["dz_interface"], land_mask=c["land_mask"], tendency_fraction=1.0, fractions=[1.0] * 4)
            Acu = dict(cu, temperature=diag["temperature"], water_vapor=s["water_vapor"], potential_temperature=s["potential_temperature"],
                       cloud_water=s["cloud_water"], cloud_ice=s["cloud_ice"], accumulated_precipitation=acc)
            B.convect(ccu, Acu, dt4, tile=tile)
        z = [np.zeros((ny, nx), np.float32) for _ in range(5)]
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
    assert n_dev == n_cpu and n_cpu >= 3, (n_dev, n_cpu)
    assert all(np.isfinite(a).all() for a in s.values())
    assert mixing > 0 and (ys["exch_h"] != 0).any(), "the scheme did something"
    assert moved > 1e-3, "rad and lsm moved the potential temperature in front of pbl: a recomputed temperature would differ"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        print(n, "differing cells:", nbitdiff(got, s[n]))
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    for k in YSU_ARRAYS:
        got = pbl.ysu_get(d, k)
        assert Y.bitdiff(got, ys[k]) == 0, f"{k}: {Y.bitdiff(got, ys[k])} of {got.size} cells differ"
    for k in B.CU_ARRAYS:
        got = convection.cu_get(d, k)
        assert bits_equal(got, cu[k]), f"{k}: {nbitdiff(got, cu[k])} of {got.size} cells differ"
    for k in S.STATE2:
        got = d.get(k)
        assert bits_equal(got, sfc[k]), f"{k}: {nbitdiff(got, sfc[k])} of {got.size} cells differ"
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    parity_record("ysu_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s})
    d.close()


def test_substep_equals_the_plain_sequence(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=72)
    opt = options(c)
    opt.lsm_options.update_interval = 100
    a, b = domain(c, dq, opt), domain(c, dq, opt)
    for n in range(2):
        substep(a, opt, dt, forced=FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474
        radiation.rad(b, opt, dt)                                             # :488
        surface.lsm(b, opt, dt)                                               # :491
        pbl.ysu_sfc(b, opt)                                                   # :494 pbl = :227-254,
        pbl.ysu(b, dt, b.its, b.ite, b.jts, b.jte, b.kts, b.kte)              #       :257-323, the tendencies left in place,
        for field, tend in (("water_vapor", "tend_qv"), ("cloud_water_mass", "tend_qc"), ("potential_temperature", "tend_th"), ("cloud_ice_mass", "tend_qi")):
            t = pbl.ysu_get(b, tend)                                          #       :343-354 by the host: x = x + tend dt in REAL(4) over the memory
            assert tend in ("tend_qc", "tend_qi") or (t != 0).any(), f"{tend} is left in place by ysu alone"
            b.set(field, (b.get(field) + t * f32(dt)).astype(f32))
        for tend in Y.TEND:
            pbl.ysu_set(b, tend, np.zeros((NY, NZ, NX), f32))
        convection.convect(b, opt, dt)                                        # :509
        CS._mp_and_halo(b, opt, dt)                                           # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, FORCED)                                           # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in OUTPUTS + R.OUTPUTS[1:] + S.STATE2:
            assert a.get(m).tobytes() == b.get(m).tobytes(), f"sub-step {n + 1}: {m}"
        for k in YSU_ARRAYS:
            assert pbl.ysu_get(a, k).tobytes() == pbl.ysu_get(b, k).tobytes(), f"sub-step {n + 1}: {k}"
    assert (pbl.ysu_get(a, "kpbl") > 1).any()
    for d in (a, b):
        d.close()


def test_2x2_tiling_equals_one_tile_in_every_owned_cell():
    c = Y.make_case(nx=40, ny=36, nz=12, seed=43, lid=4000.0)
    ny, nz, nx = c["z"].shape
    grids = [grid_t().set_grid_dimensions(nx, ny, nz, 4, im) for im in range(1, 5)]
    assert grids[0].ximages == 2 and len({(g.ims, g.jms) for g in grids}) == 4
    whole = (min(g.its for g in grids), max(g.ite for g in grids), min(g.jts for g in grids), max(g.jte for g in grids))
    names = Y.STATE3 + ["exch_h", "hpbl", "kpbl", "hol", "psim", "psih", "regime", "ri", "windspd"]
    # the one-image run, on the device ...
    d1 = Y.device_domain(c)
    assert (d1.its, d1.ite, d1.jts, d1.jte) == whole
    Y.device_call(d1, c, 0)
    one = Y.device_state(d1, names[len(Y.STATE3):])
    d1.close()
    # ... which is the restatement's
    cpu = Y.state(c)
    kept = {}
    Y.run_oracle(c, cpu, 0, tile=whole, keep=kept)
    for k in names:
        assert Y.bitdiff(one[k], cpu[k]) == 0, k
    owned = np.zeros((ny, nx), bool)
    for im, g in enumerate(grids):
        t = cut_tile(c, g); t.update(dx=c["dx"], negzero=False)
        d = Y.device_domain(t, grid=g)
        Y.device_call(d, t, 0)
        got = Y.device_state(d, names[len(Y.STATE3):])
        js, is_ = slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)
        for k in names:
            a = got[k][js, :, is_] if got[k].ndim == 3 else got[k][js, is_]
            b = one[k][g.jts - 1:g.jte, :, g.its - 1:g.ite] if one[k].ndim == 3 else one[k][g.jts - 1:g.jte, g.its - 1:g.ite]
            assert Y.bitdiff(a, b) == 0, f"image {im + 1}, {k}: the owned cells differ from the one-image run"
        owned[g.jts - 1:g.jte, g.its - 1:g.ite] = True
        d.close()
    assert owned[1:-1, 1:-1].all() and (kept["tend_th"] != 0).any()
    parity_record("ysu_step", "2x2/40x36x12", {k: {"bitdiff_cells": 0} for k in names})


def test_pbl_init_2_is_pbl_configure_2_and_0_is_never_configured(oracle):
    dt = 80.0
    c, dq = step_case(oracle, seed=73)
    simple, off = options(c, kPBL_SIMPLE, others=False), options(c, 0, others=False)

    def plain():
        d = P.device_domain(c)
        mp_init(off, d); adv_init(d, off)
        for k, x in dq.items():
            d.set_dqdt(k, x)
        return d
    by_init, by_configure, never, was_on = plain(), plain(), plain(), plain()
    check(lib().icar_hip_pbl_init(by_init.ctx, 2), "pbl_init"); by_init._pbl_key = 2
    check(lib().icar_hip_pbl_configure(by_configure.ctx, 2), "pbl_configure"); by_configure._pbl_key = 2
    pbl.pbl_init(was_on, options(c, kPBL_YSU, others=False))                  # the scheme's arrays and workspace exist ...
    pbl.pbl_finalize(off, was_on)                                            # ... and it is switched off again
    for n in range(2):
        for d, o in ((by_init, simple), (by_configure, simple), (never, off), (was_on, off)):
            substep(d, o, dt, forced=FORCED, diagnostics=True)
            d.model_time_seconds += dt
    for m in OUTPUTS:
        assert by_init.get(m).tobytes() == by_configure.get(m).tobytes(), m
        assert was_on.get(m).tobytes() == never.get(m).tobytes(), m
    assert not pbl.ysu_get(was_on, "hpbl").any() and (pbl.ysu_get(was_on, "hol") == 1000).all(), "nothing of YSU ran"
    assert by_init.get("water_vapor").tobytes() != never.get("water_vapor").tobytes(), "with pbl_simple on the result differs"
    for d in (by_init, by_configure, never, was_on):
        d.close()


def test_smoke_has_a_ysu_case_and_it_passes():
    import inspect
    import __graft_entry__ as G
    assert "smoke_ysu()" in inspect.getsource(G.smoke)
    G.smoke_ysu()

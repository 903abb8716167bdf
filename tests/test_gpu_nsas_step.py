"""The NSAS scheme in the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:509):
* icar_hip_step over three or more sub-steps with rad + lsm + YSU + NSAS + Thompson + MPDATA (exact mode) on and forced winds == the
  same loop assembled call by call on the CPU from the oracle's operators and the restatements, every prognostic field, every
  surface field and every array of the two column slots bit for bit, on 24 x 10 x 16.  NSAS reads the hpbl YSU wrote in this very
  sub-step, the temperature, w_real and mass-point winds of diagnostic_update and the surface fluxes lsm left;
* icar_hip_substep with those slots on == the plain sequence issued call by call, in which the WHOLE of diagnostic_update -- w_real
  included, which the scheme reads as W0AVG -- precedes convect;
* a 2 x 2 tiling against the restatement run tile by tile (NOT against the one-image run: kbmax, kbm and kmax are made from the
  columns of every tile row);
* convection = 0 after convection_init(ctx, 0, ..): a sub-step's outputs are byte-identical to those of a never-configured context;
* smoke() has an NSAS case and it passes."""
import numpy as np
import pytest

import nsas_oracle as N
import pbl_oracle as P
import ra_oracle as R
import sfc_oracle as S
import ysu_oracle as Y
import test_gpu_cu_step as CS
import test_gpu_ysu_step as YS
from icar_amd import radiation, pbl, surface, convection
from icar_amd.advection import advect
from icar_amd.time_step import substep, step
from icar_amd.capi import lib, check
from icar_amd.constants import kCU_NSAS, kWATER_SIMPLE, kLSM_BASIC
from icar_amd.grid import grid_t
from icar_amd.ideal import cut_tile
from util import bits_equal, nbitdiff, parity_record, MEMBER

pytestmark = pytest.mark.gpu
ADV_ORDER, FORCED, OUTPUTS, ANCHOR = CS.ADV_ORDER, CS.FORCED, CS.OUTPUTS, CS.ANCHOR
NX, NY, NZ = 24, 10, 16
RES = N.TEND + N.OUT2
f32 = np.float32


class _dims:
    """test_gpu_ysu_step's helpers on this file's 24 x 10 x 16"""
    def __enter__(self):
        self.keep = (YS.NX, YS.NY, YS.NZ)
        YS.NX, YS.NY, YS.NZ = NX, NY, NZ

    def __exit__(self, *a):
        YS.NX, YS.NY, YS.NZ = self.keep


def _case(oracle, seed):
    with _dims():
        return YS.step_case(oracle, seed)


def _options(c, ui):
    opt = YS.options(c)
    opt.physics.convection = kCU_NSAS
    opt.lsm_options.update_interval = ui
    convection.cu_var_request(opt)
    return opt


def _domain(c, dq, opt):
    with _dims():
        return YS.domain(c, dq, opt)                                          # pbl_init before init_convection, as in the reference


def _cu_state():
    cu = {k: np.zeros((NY, NZ, NX), f32) for k in N.TEND}
    cu.update({k: np.zeros((NY, NX), f32) for k in N.OUT2 + ["accumulated_convective_pcp"]})
    cu.update(diag=np.zeros((NY, NX), np.int32), limits=np.zeros((NY, 3), np.int32), own=np.zeros((NY, NX, 3), np.int32))
    return cu


def test_whole_step_loop_with_ysu_and_nsas_equals_cpu_chain(th_oracle, oracle):
    nx, ny, nz = NX, NY, NZ
    c, dq = _case(oracle, seed=81)
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    ui = max(int(1.5 * dt0), 1)
    opt = _options(c, ui)
    d = _domain(c, dq, opt)
    assert (convection.nsas_get(d, "hpbl") == 0.0).all(), "with YSU, init_convection leaves hpbl alone"
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
    cu = _cu_state()
    ys = YS.ysu_state(c)
    acc = np.zeros((ny, nx), np.float64)
    lm = c["land_mask"]
    xland = np.where((lm == 0) | (lm == 2), 2.0, lm).astype(f32)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, t_mp, moved, deep, shallow = 0.0, 0, None, 0.0, 0, 0
    tile = (2, nx - 1, 2, ny - 1)
    cf = lambda a: np.ascontiguousarray(a, f32)
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
            moved = max(moved, float(np.abs(s["potential_temperature"] * diag["exner"] - diag["temperature"]).max()))
            yc = dict(z=c["z"], dx=c["dx"], terrain=c["terrain"], land_mask=c["land_mask"], dz_interface=c["dz_interface"],        # :494 pbl, kPBL_YSU
                      ground_surf_temperature=c["ground_surf_temperature"], pressure=s["pressure"], exner=diag["exner"],
                      pressure_interface=diag["pressure_interface"], surface_pressure=diag["surface_pressure"], u_mass=diag["u_mass"], v_mass=diag["v_mass"])
            yc.update({k: A[k] for k in ("u_10m", "v_10m", "ustar", "roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")})
            yc = {k: (np.ascontiguousarray(v, np.int32 if k == "land_mask" else f32) if isinstance(v, np.ndarray) else v) for k, v in yc.items()}
            YA = dict(ys, temperature=cf(diag["temperature"]), water_vapor=s["water_vapor"], cloud_water=s["cloud_water"],
                      cloud_ice=s["cloud_ice"], potential_temperature=s["potential_temperature"])
            Y.run_sfc(yc, YA)
            Y.run_ysu(yc, YA, dt4, tile=tile)
            Y.run_apply(yc, YA, dt4)
            ys.update({k: YA[k] for k in ys})
            # :509 convect: diagnostic_update's temperature, w_real and winds, the CURRENT scalars and fluxes, the hpbl YSU just wrote
            ccu = dict(density=cf(diag["density"]), exner=cf(diag["exner"]), pressure=cf(s["pressure"]), pressure_interface=cf(diag["pressure_interface"]),
                       dz_interface=cf(c["dz_interface"]), w_real=cf(diag["w_real"]), u_mass=cf(diag["u_mass"]), v_mass=cf(diag["v_mass"]),
                       xland=xland, sensible_heat=cf(A["sensible_heat"]), latent_heat=cf(A["latent_heat"]), hpbl=cf(ys["hpbl"]), dx=c["dx"])
            Acu = dict(cu, temperature=cf(diag["temperature"]), water_vapor=s["water_vapor"], potential_temperature=s["potential_temperature"],
                       cloud_water=s["cloud_water"], cloud_ice=s["cloud_ice"], accumulated_precipitation=acc)
            N.convect(ccu, Acu, dt4, tile)
            for k in ("water_vapor", "potential_temperature", "cloud_water", "cloud_ice"):
                s[k] = Acu[k]
            deep += int((cu["diag"] & N.D_DEEP_RAIN != 0).sum()); shallow += int((cu["diag"] & N.D_SHALLOW != 0).sum())
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
    print("deep columns", deep, "shallow columns", shallow, "hpbl", float(ys["hpbl"].min()), float(ys["hpbl"].max()))
    assert deep + shallow > 0 and (cu["tend_qv"] != 0).any(), "the scheme did something"
    assert np.unique(ys["hpbl"][1:-1, 1:-1]).size > 1, "YSU's hpbl varies over the tile"
    assert moved > 1e-3, "rad and lsm moved the potential temperature in front of pbl and convect: a recomputed temperature would differ"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV_ORDER + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        print(n, "differing cells:", nbitdiff(got, s[n]))
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    got = N.device_state(d)
    for k in RES + ["accumulated_convective_pcp"]:
        assert N.bitdiff(got[k], cu[k]) == 0, f"{k}: {N.bitdiff(got[k], cu[k])} of {got[k].size} cells differ"
    for k in YS.YSU_ARRAYS:
        g = pbl.ysu_get(d, k)
        assert Y.bitdiff(g, ys[k]) == 0, f"{k}: {Y.bitdiff(g, ys[k])} of {g.size} cells differ"
    for k in S.STATE2:
        assert bits_equal(d.get(k), sfc[k]), k
    for k in R.OUTPUTS[1:]:
        assert bits_equal(d.get(k), rad2d[k]), k
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    parity_record("nsas_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s})
    d.close()


def test_substep_equals_the_plain_sequence(oracle):
    dt = 80.0
    c, dq = _case(oracle, seed=82)
    opt = _options(c, 100)
    a, b = _domain(c, dq, opt), _domain(c, dq, opt)
    for n in range(2):
        substep(a, opt, dt, forced=FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474, w_real included
        radiation.rad(b, opt, dt)                                             # :488
        surface.lsm(b, opt, dt)                                               # :491
        pbl.pbl(b, opt, dt)                                                   # :494
        convection.convect(b, opt, dt)                                        # :509
        CS._mp_and_halo(b, opt, dt)                                           # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, FORCED)                                           # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in OUTPUTS + R.OUTPUTS[1:] + S.STATE2:
            assert a.get(m).tobytes() == b.get(m).tobytes(), f"sub-step {n + 1}: {m}"
        sa, sb = N.device_state(a), N.device_state(b)
        for k in RES + ["accumulated_convective_pcp"]:
            assert sa[k].tobytes() == sb[k].tobytes(), f"sub-step {n + 1}: {k}"
        for k in YS.YSU_ARRAYS:
            assert pbl.ysu_get(a, k).tobytes() == pbl.ysu_get(b, k).tobytes(), f"sub-step {n + 1}: {k}"
    assert (sa["tend_qv"] != 0).any()
    for d in (a, b):
        d.close()


def test_2x2_tiling_equals_the_tiled_restatement():
    c = N.make_case(nx=40, ny=36, nz=24, seed=43, terrain=True, dx=4000.0)
    ny, nz, nx = c["density"].shape
    grids = [grid_t().set_grid_dimensions(nx, ny, nz, 4, im) for im in range(1, 5)]
    assert grids[0].ximages == 2 and len({(g.ims, g.jms) for g in grids}) == 4
    conv = 0
    for im, g in enumerate(grids):
        t = cut_tile(c, g); t.update(dx=c["dx"])
        d = N.device_domain(t, grid=g)
        convection.convect(d, d._cu_opt, 60.0)
        got = N.device_state(d)
        A = N.state(c)
        A["accumulated_precipitation"] = np.zeros((ny, nx), np.float64); A["accumulated_convective_pcp"] = np.zeros((ny, nx), np.float32)
        N.convect(c, A, 60.0, (g.its, g.ite, g.jts, g.jte))
        js, is_ = slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)
        for k in RES + ["water_vapor", "potential_temperature", "cloud_water", "cloud_ice"]:
            x = got[k][js, :, is_] if got[k].ndim == 3 else got[k][js, is_]
            y = A[k][g.jts - 1:g.jte, :, g.its - 1:g.ite] if A[k].ndim == 3 else A[k][g.jts - 1:g.jte, g.its - 1:g.ite]
            assert N.bitdiff(x, y) == 0, f"image {im + 1}, {k}: the owned cells differ from the restatement on this tile"
        conv += int((A["diag"][g.jts - 1:g.jte, g.its - 1:g.ite] & (N.D_DEEP_RAIN | N.D_SHALLOW) != 0).sum())
        d.close()
    assert conv > 0
    parity_record("nsas_step", "2x2/40x36x24", {k: {"bitdiff_cells": 0} for k in RES})


def test_convection_0_after_convection_init_is_a_never_configured_context(oracle):
    from icar_amd.microphysics import mp_init
    from icar_amd.advection import adv_init
    c, dq = CS.step_case(oracle, seed=83)
    off = CS.options(c, False)
    assert off.physics.convection == 0

    def plain():
        d = P.device_domain(c)
        mp_init(off, d); adv_init(d, off)
        for k, x in dq.items():
            d.set_dqdt(k, x)
        return d
    never, zero, was_on = plain(), plain(), plain()
    convection.convection_init(zero, 0, dx=0.0)                              # dx is ignored
    convection.convection_init(was_on, 4)                                    # the scheme's arrays and workspace exist ...
    convection.convection_init(was_on, 0)                                    # ... and the slot is switched off again
    for n in range(2):
        for d in (never, zero, was_on):
            substep(d, off, 80.0, forced=FORCED, diagnostics=True)
            d.model_time_seconds += 80.0
    for m in OUTPUTS:
        assert zero.get(m).tobytes() == never.get(m).tobytes(), m
        assert was_on.get(m).tobytes() == never.get(m).tobytes(), m
    assert not convection.cu_get(was_on, "raincv").any() and not convection.nsas_get(was_on, "pratec").any(), "nothing ran"
    for d in (never, zero, was_on):
        d.close()


def test_smoke_has_an_nsas_case_and_it_passes():
    import inspect
    import __graft_entry__ as G
    assert "smoke_nsas()" in inspect.getsource(G.smoke)
    G.smoke_nsas()

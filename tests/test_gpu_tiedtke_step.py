"""The Tiedtke scheme in the sub-step loop (icar_amd/csrc/timestep.hip; time_step.f90:509):
* icar_hip_step over three or more sub-steps with rad + lsm + pbl + Tiedtke + Thompson + MPDATA (exact mode) on and forced winds ==
  the same loop assembled call by call on the CPU from the oracle's operators and the restatements, every prognostic field, every
  surface field and every array of the scheme bit for bit, on 24 x 20 x 20;
* icar_hip_substep with rad + lsm + pbl + Tiedtke + Thompson + MPDATA on == the plain sequence issued call by call, in which the
  WHOLE of diagnostic_update -- w_real included, which the scheme reads as W0AVG -- precedes convect;
* a 2 x 2 tiling against the restatement run tile by tile (NOT against the one-image run: leveltop is made from the first column of
  every tile row);
* smoke() has a Tiedtke case and it passes.
"""
import numpy as np
import pytest

import pbl_oracle as P
import ra_oracle as R
import sfc_oracle as S
import tiedtke_oracle as T
from icar_amd import radiation, pbl, surface, convection
from icar_amd.microphysics import mp_init
from icar_amd.advection import advect, adv_init
from icar_amd.time_step import substep, step
from icar_amd.capi import lib, check
from icar_amd.constants import kWATER_SIMPLE, kLSM_BASIC
from util import bits_equal, nbitdiff, MEMBER
from icar_amd.constants import kCU_TIEDTKE
from icar_amd.grid import grid_t
from icar_amd.ideal import cut_tile
from util import parity_record
import test_gpu_cu_step as BS

pytestmark = pytest.mark.gpu
RES = T.TEND + T.OUT2 + ["ktype"]


def _domain(c, dq, opt):
    d = P.device_domain(c)
    d.znu = c["znu"]
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((BS.NY, BS.NX), R.SENTINEL, np.float32))
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt); surface.lsm_init(d, opt)
    convection.init_convection(d, opt)
    radiation.rad_calendar(d, *BS.ANCHOR)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d


def _znu():
    return ((np.arange(BS.NZ, 0, -1) - 0.5) / BS.NZ).astype(np.float32)


def test_whole_step_loop_with_every_slot_equals_cpu_chain(th_oracle, oracle):
    nx, ny, nz = BS.NX, BS.NY, BS.NZ
    ADV = BS.ADV_ORDER
    c, dq = BS.step_case(oracle, seed=61)
    c["znu"] = _znu()
    f32 = np.float32
    dt0 = min(float(f32(0.9) / f32(oracle.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)
    ui = max(int(1.5 * dt0), 1)
    opt = BS.options(c, True, update_interval=ui, cu=kCU_TIEDTKE)
    d = _domain(c, dq, opt)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    end = 3.4 * dt0
    n_dev = step(d, end, opt, forced=BS.FORCED, diagnostics=True)
    s = {k: c[k].copy() for k in ADV + ["u", "v", "w", "pressure"]}
    rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
    sfc = {k: c[k].copy() for k in ("roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")}
    sfc.update(u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32),
               qsfc=c["water_vapor"][:, 0, :].copy(), qfx=np.zeros((ny, nx), f32), last_model_time=-999.0)
    par = dict(watersurface=kWATER_SIMPLE, landsurface=kLSM_BASIC, sfc_layer_thickness=400.0, sh_feedback_fraction=0.625, lh_feedback_fraction=1.0,
               update_interval=ui, kts=1)
    cu = {k: np.zeros((ny, nz, nx), f32) for k in T.TEND}
    cu.update(raincv=np.zeros((ny, nx), f32), pratec=np.zeros((ny, nx), f32), accumulated_convective_pcp=np.zeros((ny, nx), f32),
              ktype=np.zeros((ny, nx), np.int32), diag=np.zeros((ny, nx), np.int32))
    acc = np.zeros((ny, nx), np.float64)
    lm = c["land_mask"]
    xland = np.where((lm == 0) | (lm == 2), 2.0, lm).astype(f32)
    th_oracle.set_math_mode(0); oracle.set_math_mode(0)
    t, n_cpu, t_mp, moved, convecting = 0.0, 0, None, 0.0, 0
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
            D, yd = BS.day_of_year(t)                                                                   # :488 rad
            Ar = dict(rad2d); Ar["potential_temperature"] = s["potential_temperature"]
            inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
            R.ra_simple(Ar, inputs, D, yd, BS.ANCHOR[0], dt4, 2, nx - 1, 2, ny - 1, 1, nz)
            if S.gate(cc, A, t): S.water_simple(cc, A)                                                  # :491 lsm
            S.apply_fluxes(cc, A, dt4)
            sfc["last_model_time"] = A["last_model_time"]
            P.simple_pbl({k: s[k] for k in P.SCALARS}, diag["u_mass"], diag["v_mass"], diag["exner"], diag["density"], c["z"], c["dz_mass"],   # :494 pbl
                         c["terrain"], c["land_mask"], 2, nx - 1, 2, ny - 1, 1, nz, dt4)
            # :509 convect: the temperature and w_real of diagnostic_update, the CURRENT water vapour, cloud water, cloud ice and theta
            moved = max(moved, float(np.abs(s["potential_temperature"] * diag["exner"] - diag["temperature"]).max()))
            ccu = dict(density=diag["density"], exner=diag["exner"], pressure=s["pressure"], pressure_interface=diag["pressure_interface"],
                       dz_interface=c["dz_interface"], w_real=diag["w_real"], xland=xland, znu=c["znu"])
            Acu = dict(cu, temperature=diag["temperature"], water_vapor=s["water_vapor"], potential_temperature=s["potential_temperature"],
                       cloud_water=s["cloud_water"], cloud_ice=s["cloud_ice"], accumulated_precipitation=acc)
            T.convect(ccu, Acu, dt4, (2, nx - 1, 2, ny - 1))
            convecting += int((cu["ktype"] == 3).sum())
        z = [np.zeros((ny, nx), np.float32) for _ in range(5)]
        mp_dt = dt4 if t_mp is None else float(f32(t - t_mp)); t_mp = t
        th_oracle.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"],
                           s["rain_number"], s["potential_temperature"], diag["exner"], s["pressure"], c["dz_mass"], mp_dt, *z,
                           1, nx, 1, ny, 1, nz, 2, nx - 1, 2, ny - 1, 1, nz)
        acc += z[0]
        q = np.stack([s[n] for n in ADV]).copy()
        oracle.advect(2, q, s["u"], s["v"], s["w"], diag["density"], c["jacobian"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"],
                      c["advection_dz"], c["dz_levels"], float(c["dx"]), dt4)
        for m, n in enumerate(ADV): s[n] = q[m].copy()
        for n, fb in BS.FORCED:
            oracle.apply_forcing(s[n], dq[n], dt, int(fb), 1, 1, 1, 1)
        if enforce:
            for n in ADV: oracle.enforce_limits(s[n])
        t += dt; n_cpu += 1
    assert n_dev == n_cpu and n_cpu >= 3, (n_dev, n_cpu)
    assert all(np.isfinite(a).all() for a in s.values())
    assert convecting > 0 and (cu["tend_qv"] != 0).any(), "the scheme did something"
    assert moved > 1e-3, "rad, lsm and pbl moved the potential temperature in front of convect: a recomputed temperature would differ"
    dev_name = dict(MEMBER); dev_name.update({"u": "u", "v": "v", "w": "w", "pressure": "pressure"})
    for n in ADV + ["u", "v", "w", "pressure"]:
        got = d.get(dev_name[n])
        print(n, "differing cells:", nbitdiff(got, s[n]))
        assert bits_equal(got, s[n]), f"{n}: {nbitdiff(got, s[n])} of {got.size} cells differ after {n_cpu} sub-steps"
    got = T.device_state(d)
    for k in RES + ["accumulated_convective_pcp"]:
        assert T.bitdiff(got[k], cu[k]) == 0, f"{k}: {T.bitdiff(got[k], cu[k])} of {got[k].size} cells differ"
    for k in S.STATE2:
        assert bits_equal(d.get(k), sfc[k]), k
    for k in R.OUTPUTS[1:]:
        assert bits_equal(d.get(k), rad2d[k]), k
    assert np.array_equal(d.get("accumulated_precipitation"), acc)
    parity_record("tiedtke_step", f"whole_step_loop/{nx}x{ny}x{nz}/exact_mode_{n_cpu}_substeps", {n: {"bitdiff_cells": 0, "cells": int(s[n].size)} for n in s})
    d.close()


def test_substep_equals_the_plain_sequence(oracle):
    dt = 80.0
    c, dq = BS.step_case(oracle, seed=62)
    c["znu"] = _znu()
    opt = BS.options(c, True, update_interval=100, cu=kCU_TIEDTKE)
    domain = lambda: _domain(c, dq, opt)
    a, b = domain(), domain()
    for n in range(2):
        substep(a, opt, dt, forced=BS.FORCED, diagnostics=True)
        b.diagnostic_update(3)                                                # time_step.f90:474, w_real included
        radiation.rad(b, opt, dt)                                             # :488
        surface.lsm(b, opt, dt)                                               # :491
        pbl.pbl(b, opt, dt)                                                   # :494
        convection.convect(b, opt, dt)                                        # :509
        BS._mp_and_halo(b, opt, dt)                                           # :512-526
        advect(b, opt, dt)                                                    # :529
        b.apply_forcing(dt, BS.FORCED)                                        # :534
        for d in (a, b):
            d.model_time_seconds += dt
        for m in BS.OUTPUTS + R.OUTPUTS[1:] + S.STATE2:
            assert a.get(m).tobytes() == b.get(m).tobytes(), f"sub-step {n + 1}: {m}"
        sa, sb = T.device_state(a), T.device_state(b)
        for k in RES + ["accumulated_convective_pcp"]:
            assert sa[k].tobytes() == sb[k].tobytes(), f"sub-step {n + 1}: {k}"
    assert (sa["tend_qv"] != 0).any()
    for d in (a, b):
        d.close()


def test_2x2_tiling_equals_the_tiled_restatement():
    c = T.make_case(nx=40, ny=36, nz=24, seed=43, terrain=True, depth_max=8000.0)
    ny, nz, nx = c["density"].shape
    grids = [grid_t().set_grid_dimensions(nx, ny, nz, 4, im) for im in range(1, 5)]
    assert grids[0].ximages == 2 and len({(g.ims, g.jms) for g in grids}) == 4
    conv = 0
    for im, g in enumerate(grids):
        t = cut_tile(c, g); t.update(znu=c["znu"], dx=c["dx"])
        d = T.device_domain(t, grid=g)
        convection.convect(d, d._cu_opt, 60.0)
        got = T.device_state(d)
        A = T.state(c)
        A["accumulated_precipitation"] = np.zeros((ny, nx), np.float64); A["accumulated_convective_pcp"] = np.zeros((ny, nx), np.float32)
        T.convect(c, A, 60.0, (g.its, g.ite, g.jts, g.jte))
        js, is_ = slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)
        for k in RES + ["water_vapor", "potential_temperature", "cloud_water", "cloud_ice"]:
            x = got[k][js, :, is_] if got[k].ndim == 3 else got[k][js, is_]
            y = A[k][g.jts - 1:g.jte, :, g.its - 1:g.ite] if A[k].ndim == 3 else A[k][g.jts - 1:g.jte, g.its - 1:g.ite]
            assert T.bitdiff(x, y) == 0, f"image {im + 1}, {k}: the owned cells differ from the restatement on this tile"
        conv += int((A["ktype"] == 3).sum())
        d.close()
    assert conv > 0
    parity_record("tiedtke_step", "2x2/40x36x24", {k: {"bitdiff_cells": 0} for k in RES})


def test_smoke_has_a_tiedtke_case_and_it_passes():
    import inspect
    import __graft_entry__ as G
    assert "smoke_tiedtke()" in inspect.getsource(G.smoke)
    G.smoke_tiedtke()

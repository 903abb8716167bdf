"""First measurement of the forcing step (profiles/r20_steps.md): icar_hip_forcing_step at 512 x 512 x 40 from a 64 x 30 x 64 forcing grid
with nine forced 3-D fields (seven scalars sharing the mass tables, u, v), by the library's HIP-event timers, group by group; the
pressure path (k_forcing_mass_novert + k_adjust_pressure) from a 64 x 40 x 64 grid beside it; and what it replaces: icar_hip_field_download
of the nine fields and icar_hip_dqdt_download of three tendencies, then field_upload / dqdt_upload of the same.
    python profiles/micro/forcing_time.py [out.json]
The tables are geometric (neighbouring columns name neighbouring forcing cells), not random: the gather's cache behaviour is a run's."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from icar_amd import forcing as F  # noqa: E402
from icar_amd.capi import lib, check  # noqa: E402
from icar_amd.domain import domain_t  # noqa: E402
from icar_amd.grid import grid_t  # noqa: E402
from icar_amd.options import options_t  # noqa: E402

f32 = np.float32
NX, NZ, NY = 512, 40, 512
SCALARS = ["water_vapor", "potential_temperature", "cloud_water_mass", "rain_mass", "snow_mass", "cloud_ice_mass", "graupel_mass"]


def tables(rng, nx, ny, nz, nxf, nzf, nyf, i0=0, j0=0):
    a = (np.arange(nx) + 0.5) * (nxf - 1) / nx
    b = (np.arange(ny) + 0.5) * (nyf - 1) / ny
    x1 = np.floor(a).astype(np.int32) + 1
    y1 = np.floor(b).astype(np.int32) + 1
    x = np.broadcast_to(np.stack([x1, x1 + 1, x1, x1 + 1], -1)[None], (ny, nx, 4))
    y = np.broadcast_to(np.stack([y1, y1, y1 + 1, y1 + 1], -1)[:, None], (ny, nx, 4))
    w = rng.random((ny, nx, 4)).astype(f32)
    zc = (np.arange(nz) + 0.5) * (nzf - 1) / nz
    z1 = np.floor(zc).astype(np.int32) + 1
    z = np.broadcast_to(np.stack([z1, z1 + 1], -1)[None, :, None], (ny, nz, nx, 2))
    zw = rng.random((ny, nz, nx, 2)).astype(f32)
    return dict(x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), w=w, z=np.ascontiguousarray(z), zw=zw, i0=i0, j0=j0)


def read(d, group):
    ms, n = ctypes.c_double(), ctypes.c_int()
    check(lib().icar_hip_timing_read(d.ctx, group.encode(), ctypes.byref(ms), ctypes.byref(n)), "timing_read")
    return ms.value, n.value


def run(nzf, with_pressure):
    rng = np.random.default_rng(1)
    nxf, nyf, ns, e = 64, 64, 2, 2
    sf = (nyf, nzf, nxf)
    g = tables(rng, NX, NY, NZ, nxf, nzf, nyf)
    gu = tables(rng, NX + 1 + 2 * e, NY + 2 * e, NZ, nxf, nzf, nyf, e, e)
    gv = tables(rng, NX + 2 * e, NY + 1 + 2 * e, NZ, nxf, nzf, nyf, e, e)
    keys = ("x", "y", "w", "z", "zw")
    geo_z = np.cumsum(rng.uniform(100, 600, (NY, nzf, NX)), axis=1).astype(f32)
    z = np.cumsum(rng.uniform(100, 400, (NY, NZ, NX)), axis=1).astype(f32)
    names = SCALARS + ["u", "v"] + (["pressure"] if with_pressure else [])
    lo = {n: rng.uniform(280.0, 320.0, sf).astype(f32) for n in names}
    if with_pressure: lo["pressure"] = rng.uniform(3e4, 1e5, sf).astype(f32)
    b = F.boundary_t(F.geo_t(*(g[k] for k in keys), forcing_shape=sf, geo_z=geo_z), F.geo_t(*(gu[k] for k in keys), forcing_shape=sf, i0=e, j0=e),
                     F.geo_t(*(gv[k] for k in keys), forcing_shape=sf, i0=e, j0=e), lo)
    d = domain_t(grid_t().set_grid_dimensions(NX, NY, NZ, 1, 1), device=0, dx=2000.0)
    F.forcing_configure(d, b, ns, domain_z=z if with_pressure else None)
    for k, s in (("jacobian", (NY, NZ, NX)), ("jacobian_u", (NY, NZ, NX + 1)), ("jacobian_v", (NY + 1, NZ, NX)), ("jacobian_w", (NY, NZ, NX)), ("advection_dz", (NY, NZ, NX))):
        d.set(k, rng.uniform(0.9, 1.1, s).astype(f32) * (200.0 if k == "advection_dz" else 1.0))
    d.set("sintheta", np.zeros((NY, NX))); d.set("costheta", np.ones((NY, NX)))
    d.interpolate_forcing(b, update=False)
    d.set("w", np.zeros((NY, NZ, NX), f32))
    opt = options_t(); opt.physics.windtype = 0
    out = {}
    for rep in range(3):                                          # the last repetition is reported (the first pays the allocations)
        check(lib().icar_hip_timing_reset(d.ctx), "timing_reset"); check(lib().icar_hip_timing_enable(d.ctx, 1), "timing_enable")
        t0 = time.perf_counter()
        F.forcing_step(d, b, opt, 3600.0)
        d.synchronize()
        wall = time.perf_counter() - t0
        check(lib().icar_hip_timing_enable(d.ctx, 0), "timing_enable")
        out = {"wall_ms_with_uploads": wall * 1e3}
        for grp in ("interpolate_forcing", "forcing_mass", "forcing_wind", "forcing_pressure", "update_delta_fields"):
            out[grp + "_ms"], out[grp + "_launches"] = read(d, grp)
    n3 = NX * NZ * NY
    nm = len(SCALARS)
    # compulsory bytes of k_forcing_mass: the vert_lut entry once (16 B / cell), per variable the 4 B written; the geolut per column
    out["forcing_mass_bytes"] = n3 * (16 + 4 * nm) + NX * NY * 44
    out["forcing_mass_GBps"] = out["forcing_mass_bytes"] / (out["forcing_mass_ms"] * 1e-3) / 1e9 if out["forcing_mass_ms"] else None
    out["update_delta_bytes"] = 12 * n3 * (len(names) + 1)
    out["update_delta_GBps"] = out["update_delta_bytes"] / (out["update_delta_fields_ms"] * 1e-3) / 1e9 if out["update_delta_fields_ms"] else None
    if not with_pressure:
        # the alternative: the forced fields and three tendencies down, the same up
        host = {n: np.empty(d.shape(d.fid(n)), f32) for n in names}
        d.synchronize()
        t0 = time.perf_counter()
        for n in names: host[n] = d.get(n)
        tend = {n: d.get_dqdt(n) for n in ("u", "v", "w")}
        t1 = time.perf_counter()
        for n in names: d.set(n, host[n])
        for n in tend: d.set_dqdt(n, tend[n])
        d.synchronize()
        t2 = time.perf_counter()
        out["alternative_download_ms"], out["alternative_upload_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        out["alternative_bytes_each_way"] = int(sum(h.nbytes for h in host.values()) + sum(t.nbytes for t in tend.values()))
    d.close()
    return out


if __name__ == "__main__":
    res = {"tile": [NX, NZ, NY], "nine_fields_64x30x64": run(30, False), "with_pressure_64x40x64": run(40, True)}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)

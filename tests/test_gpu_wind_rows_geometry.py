"""The linear-wind rows W2 and W3 (icar_amd/csrc/linear_winds.hip) at every edge of their launch geometry and of the look-up table;
tests/test_gpu_winds.py has them at one interior shape per entry point.

W2 (spatial_winds): widths that put nx and nx + 1 on both sides of 64 and 128 (k_lw_nsq, k_lw_vsmooth, k_lw_rowmeans over nx;
k_lw_means, k_lw_interp over nx + 1), level counts on every nz % 4 and beyond 64 (the tiles of 4 levels, the second block of
k_lw_colsmooth), n3 on and off a multiple of 256 (k_lw_exp), row counts on both sides of the smoothing window (the arms of the
running row sums), vertical windows cut off at the top, the bottom and both ends, every combination of variable_N and
smooth_nsq, hydrometeor fields present / absent / only one, update on and off, two passes, and the smallest axes the setup takes.
A planted case walks the bracket search and calc_weight through their edges: calm faces, v == 0 with either sign of u, a
direction on 0, on pi and on dirmax, a speed on an axis value and beyond spdmax, N^2 on both clamps, and -- with a second set of
options whose axes end inside the data -- match < d(1) and bestpos == n on all three axes.  Every comparison is bit for bit,
against the C oracle (oracle/wind_oracle.c) AND against the numpy restatement of the Fortran statements
(tests/wind_rows_case.py; tests/test_wind_rows_inputs.py holds the two to each other without a GPU, and counts the branches):
these are FP32 statements in the reference's order with the restated libm, so the number is 0 differing bits and there is no
tolerance to choose.

W3 (terrain spectrum, perturbation, table build): odd, prime and mixed transform sizes (the reference shifts by (n + 1) / 2, and
fftshift is not its own inverse for odd n), the constant-z table on every image of two decompositions with bit-identical
overlaps, the space_varying_dz table on tiles with a non-zero offset and differing sub-layer counts, and nx + 1 on 64 / 65 (the
block edge of both destagger kernels and both directions of k_lut_transpose).  Tolerances are the ones of test_gpu_winds.py; the
measured errors go to the parity record.

Not tested: the level chunking of icar_linwinds_build_lut_run (plan slot 1, a last chunk shorter than the others).  It only
happens above 4 GB of spectrum, which no small shape reaches."""
import numpy as np
import pytest
import util
import wind_rows_case as S
from icar_amd import linear_winds as LW
from icar_amd.capi import IcarHipError
from icar_amd.domain import domain_t
from icar_amd.grid import grid_t
from icar_amd.options import options_t
from oracle import wind_oracle as W
from util import bits_equal, nbitdiff, parity_record
from wind_case import terrain, lut_options

pytestmark = pytest.mark.gpu
f32 = np.float32
RECORD = "wind_rows_geometry"
STATE = ("z", "potential_temperature", "exner", "water_vapor", "cloud_water_mass", "cloud_ice_mass", "rain_mass", "snow_mass")


def make_domain(nx, ny, nz, dx, nimages=1, image=1):
    return domain_t(grid_t().set_grid_dimensions(nx, ny, nz, nimages, image), device=0, dx=dx)


def same(got, want, what):
    if not bits_equal(got, want):
        at = np.argwhere(np.ascontiguousarray(got).view(np.int32) != np.ascontiguousarray(want).view(np.int32))[0]
        raise AssertionError(f"{what}: {nbitdiff(got, want)} of {got.size} differ, first at (j, k, i) = {tuple(int(a) for a in at)}, "
                             f"got {got[tuple(at)]!r}, want {want[tuple(at)]!r}")


def w2_domain(c, x):
    """a single-image domain with the case's fields and random tables on the device"""
    a, lt = x["a"], x["lt"]
    opt = options_t(); opt.lt_options = lt
    d = make_domain(c["nx"], c["ny"], c["nz"], 1000.0)
    LW.setup_linwinds(d, opt, terrain(c["nx"], c["ny"]), build=False)
    LW.lut_upload(d, opt, 0, x["ulut"]); LW.lut_upload(d, opt, 1, x["vlut"])
    for k in STATE:
        if k in a:
            d.set(k, a[k])
    if c["update"]:
        d.set("u", np.zeros_like(a["u"])); d.set("v", np.zeros_like(a["v"]))
        d.set_dqdt("u", a["u"]); d.set_dqdt("v", a["v"])
    else:
        d.set("u", a["u"]); d.set("v", a["v"])
    return d, opt


def device_run(c, x):
    d, opt = w2_domain(c, x)
    try:
        for _ in range(S.PASSES):
            LW.linear_perturb(d, opt, x["lt"].vert_smooth, False, False, update=c["update"])
        if c["update"]:
            # the targets are the dqdt mirrors: recover them through apply_forcing onto the zeroed u, v (x += dqdt * 1)
            d.apply_forcing(1.0, [("u", False), ("v", False)])
        return d.get("u"), d.get("v"), LW.perturbation_download(d, 0), LW.perturbation_download(d, 1), d.get("nsquared")
    finally:
        d.close()


def check_case(oracle, c, faces=None):
    """the five fields of the case after both passes: device == oracle == restatement.  faces = [(row, face)]: those faces (all
    levels) are compared first and on their own, so that a failure names the planted branch"""
    x = S.inputs(c)
    oracle.set_math_mode(0)              # logf / expf / atanf of the C library, as the compiled reference calls them
    want = S.run(oracle.spatial_winds, c, x)
    mine = S.run(S.spatial_winds, c, x)
    got = device_run(c, x)
    for r, face in faces or ():
        for m in range(4):               # u and its perturbation at the face, v and its perturbation at the cell the face reads
            i = face if m % 2 == 0 else min(face, c["nx"] - 1)
            same(got[m][r, :, i], want[m][r, :, i], f"{c['label']} {S.FIELDS[m]} at planted row {r} face {face} vs oracle")
    for n, g, w, m in zip(S.FIELDS, got, want, mine):
        assert np.isfinite(g).all(), f"{c['label']} {n}: not finite"
        same(g, w, f"{c['label']} {n} vs oracle")
        same(g, m, f"{c['label']} {n} vs restatement")
    assert abs(got[2]).max() > 0.1
    parity_record(RECORD, f"spatial_winds/{c['label']} {c['nx']}x{c['ny']}x{c['nz']}",
                  {n: {"bitdiff_cells": 0, "cells": int(g.size)} for n, g in zip(S.FIELDS, got)})


@pytest.mark.parametrize("cases", [S.width_cases, S.level_cases, S.row_cases, S.window_cases, S.unsmoothed_cases])
def test_spatial_winds_sweep(oracle, cases):
    for c in cases():
        check_case(oracle, c)


@pytest.mark.parametrize("second", [False, True])
def test_planted_bracket_edges(oracle, second):
    c = S.planted_case(second)
    check_case(oracle, c, faces=[(r, face) for r in S.PLANT_ROWS for face in S.PLANT_FACES])


def test_refusal_leaves_the_state_alone(oracle):
    """smooth_array's rowmeans(2:windowsize) needs nx > stability_window_size: with smooth_nsq on the device refuses nx == winsz
    before it writes anything; with smooth_nsq off the same shape runs"""
    c = S.case("refused 4 wide winsz 4", 4, 3, 3, 4, 1, 30, variable_N=True, smooth_nsq=True)
    assert not c["update"] and c["nx"] == c["winsz"]
    x = S.inputs(c)
    a = x["a"]
    rng = np.random.default_rng(8)
    before = {"u": a["u"], "v": a["v"], "nsquared": rng.uniform(1e-6, 1e-4, a["z"].shape).astype(np.float32),
              "up": rng.standard_normal(a["u"].shape).astype(np.float32), "vp": rng.standard_normal(a["v"].shape).astype(np.float32)}
    d, opt = w2_domain(c, x)
    d.set("nsquared", before["nsquared"])
    LW.perturbation_upload(d, 0, before["up"]); LW.perturbation_upload(d, 1, before["vp"])
    with pytest.raises(IcarHipError, match="smooth_array needs nx > stability_window_size"):
        LW.linear_perturb(d, opt, 1, False, False, update=False)
    after = {"u": d.get("u"), "v": d.get("v"), "nsquared": d.get("nsquared"), "up": LW.perturbation_download(d, 0),
             "vp": LW.perturbation_download(d, 1)}
    d.close()
    for k, w in before.items():
        same(after[k], w, f"{k} after the refusal")
    parity_record(RECORD, "refusal 4x3x3", {k: {"bitdiff_cells": 0, "cells": int(w.size)} for k, w in before.items()})
    check_case(oracle, S.case("4 wide winsz 4 unsmoothed", 4, 3, 3, 4, 1, 30, variable_N=True, smooth_nsq=False))


# ---- W3 -----------------------------------------------------------------------------------------------------------------------
def w3_domain(nxg, nyg, buffer, nimages=1, image=1, build=True, varying=None, seed=4):
    t = terrain(nxg, nyg, seed=seed)
    opt = options_t(); opt.lt_options = S.w3_options(buffer)
    opt.parameters.dz_levels = S.DZ_LEVELS.copy()
    d = make_domain(nxg, nyg, len(S.DZ_LEVELS), S.W3_DX, nimages, image)
    if varying is not None:
        opt.parameters.space_varying_dz = True
        LW.setup_linwinds(d, opt, t, global_z_bottom=varying[0], global_z_top=varying[1])
    else:
        LW.setup_linwinds(d, opt, t, build=build)
    return d, opt, t


def tile_slices(d, ul, vl):
    """the part of the global oracle tables [s, d, n, i, z, j] that the image holds, in the device's download order"""
    i0, j0 = d.grid.ims - 1, d.grid.jms - 1
    return (np.ascontiguousarray(ul[:, :, :, i0:i0 + d.nx + 1, :, j0:j0 + d.ny].transpose(5, 4, 3, 2, 1, 0)),
            np.ascontiguousarray(vl[:, :, :, i0:i0 + d.nx, :, j0:j0 + d.ny + 1].transpose(5, 4, 3, 2, 1, 0)))


def lut_close(got, want, label):
    """within the project's 1e-5 max|LUT|; the measured maximum goes to the parity record"""
    util.COUNTS["tolerance_fields"] += 1
    assert got.shape == want.shape and np.isfinite(got).all(), label
    scale = float(abs(want).max())
    assert scale > 0.05, label
    err = float(abs(got.astype(np.float64) - want).max()) / scale
    parity_record(RECORD, label, {"lut": {"max_abs_over_max": err, "bitdiff_frac": float((got != want).mean()), "cells": int(got.size)}})
    assert err <= 1e-5, f"{label}: {err:.3e} of max|LUT|"


@pytest.mark.parametrize("size", S.W3_SIZES)
def test_terrain_spectrum_and_perturbation_at_odd_sizes(size):
    nxg, nyg, buffer = size
    fx, fy = S.transform_size(*size)
    d, opt, t = w3_domain(nxg, nyg, buffer, build=False)
    try:
        tf, lt, buf = W.setup_linwinds(t.T.copy(), S.W3_DX, buffer)
        got = LW.terrain_frequency(d)                                   # [fftny, fftnx]
        assert got.shape == (fy, fx) and tf.shape == (fx, fy)
        amp = abs(tf).max()
        util.COUNTS["tolerance_fields"] += 1
        # identical up to one single-precision ulp of each coefficient (the single-precision temp of the reference's fftshift)
        err = abs(got.T - tf)
        stats = {"terrain_frequency": {"identical_frac": float((got.T == tf).mean()), "max_abs_over_max": float(err.max() / amp),
                                       "max_over_allowed": float((err / (1.3e-7 * abs(tf) + 1e-12 * amp)).max()), "cells": int(tf.size)}}
        print(f"{fx} x {fy}: {stats}")
        assert np.all(err <= 1.3e-7 * abs(tf) + 1e-12 * amp), stats
        for (U, V, nsq, zb, zt) in S.PERTURBATIONS:
            gu, gv = LW.linear_perturbation(d, U, V, nsq, zb, zt, 100.0, got.shape)
            # feed the oracle the device's terrain spectrum so that the comparison isolates this routine
            ou, ov = W.linear_perturbation_constz(U, V, nsq, zb, zt, 100.0, got.T.copy(), lt)
            for name, g, o in (("u", gu, ou), ("v", gv, ov)):
                util.COUNTS["tolerance_fields"] += 1
                scale = abs(o.real).max()
                assert scale > 1e-3 and np.isfinite(g).all()
                e = float(abs(g.T - o.real).max() / scale)
                stats[f"{name}_perturbation U={U} V={V} Nsq={nsq}"] = {"max_abs_over_max": e, "cells": int(g.size)}
                assert e <= 1e-9, (size, U, V, name, e)
        gu, gv = LW.linear_perturbation(d, 0.0, 0.0, 1e-4, 0.0, 100.0, 100.0, got.shape)
        assert not gu.any() and not gv.any()
        parity_record(RECORD, f"spectrum {fx}x{fy}", stats)
    finally:
        d.close()


@pytest.mark.parametrize("nimages", S.TILINGS)
def test_constant_z_lut_on_every_image(nimages):
    nxg, nyg, buffer = S.TILED
    t = terrain(nxg, nyg, seed=4)
    tf, lt, buf = W.setup_linwinds(t.T.copy(), S.W3_DX, buffer)
    zb, zt = S.layer_bounds()
    ul, vl, *_ = W.build_lut(tf, lt, buf, zb, zt, lut_options(S.w3_options(buffer)))
    nz = len(zb)
    nd, ns, nn = S.W3_AXES
    # what the images hold on the global grid: an overlap (neighbours share two cells) must carry the same bits, since every
    # image runs the same transform on the same spectrum
    glob = [np.zeros((nyg, nz, nxg + 1, nn, nd, ns), np.float32), np.zeros((nyg + 1, nz, nxg, nn, nd, ns), np.float32)]
    seen = [np.zeros(g.shape[:3:2], bool) for g in glob]
    shared = [0, 0]
    for image in range(1, nimages + 1):
        d, opt, _ = w3_domain(nxg, nyg, buffer, nimages, image)
        try:
            got = (LW.lut_download(d, opt, 0), LW.lut_download(d, opt, 1))
            i0, j0 = d.grid.ims - 1, d.grid.jms - 1
        finally:
            d.close()
        for comp, (g, w) in enumerate(zip(got, tile_slices(d, ul, vl))):
            lut_close(g, w, f"constant z {nimages} images, image {image} comp {comp}")
            rows, cols = slice(j0, j0 + g.shape[0]), slice(i0, i0 + g.shape[2])
            old = seen[comp][rows, cols]
            if old.any():
                a = g.transpose(0, 2, 1, 3, 4, 5)[old]; b = glob[comp][rows, :, cols].transpose(0, 2, 1, 3, 4, 5)[old]
                same(a, b, f"{nimages} images: image {image} comp {comp} on the faces it shares with earlier images")
                shared[comp] += int(old.sum())
            glob[comp][rows, :, cols] = g
            seen[comp][rows, cols] = True
    assert all(s.all() for s in seen) and min(shared) > 0
    parity_record(RECORD, f"constant z {nimages} images overlap", {"uLUT": {"bitdiff_cells": 0, "cells": shared[0] * nz * nd * ns * nn},
                                                                   "vLUT": {"bitdiff_cells": 0, "cells": shared[1] * nz * nd * ns * nn}})


@pytest.mark.parametrize("size", S.W3_SIZES[3:])
def test_lut_at_nx_plus_1_on_64_and_65(size):
    nxg, nyg, buffer = size
    d, opt, t = w3_domain(nxg, nyg, buffer)
    try:
        assert d.nx + 1 in (64, 65)
        tf, lt, buf = W.setup_linwinds(t.T.copy(), S.W3_DX, buffer)
        zb, zt = S.layer_bounds()
        ul, vl, *_ = W.build_lut(tf, lt, buf, zb, zt, lut_options(opt.lt_options))
        got = (LW.lut_download(d, opt, 0), LW.lut_download(d, opt, 1))
        nd, ns, nn = S.W3_AXES
        for comp, (g, w) in enumerate(zip(got, tile_slices(d, ul, vl))):
            lut_close(g, w, f"{nxg}x{nyg} comp {comp}")
            # one entry as the device holds it == the slice of the transposed download, for every entry
            for k in range(ns):
                for i in range(nd):
                    for j in range(nn):
                        same(LW.lut_entry(d, comp, k, i, j), np.ascontiguousarray(g[..., j, i, k]), f"{nxg}x{nyg} lut_entry comp {comp} ({k}, {i}, {j})")
            assert not g[..., 0].any()                                  # spd = 0 entries
            # upload / download round trip in the reference's index order
            r = np.random.default_rng(comp).standard_normal(g.shape).astype(np.float32)
            LW.lut_upload(d, opt, comp, r)
            same(LW.lut_download(d, opt, comp), r, f"{nxg}x{nyg} round trip comp {comp}")
            same(LW.lut_entry(d, comp, ns - 1, nd - 1, nn - 1), np.ascontiguousarray(r[..., nn - 1, nd - 1, ns - 1]), f"{nxg}x{nyg} uploaded entry comp {comp}")
            parity_record(RECORD, f"lut_entry and round trip {nxg}x{nyg} comp {comp}", {"lut": {"bitdiff_cells": 0, "cells": int(g.size)}})
    finally:
        d.close()


def test_space_varying_dz_lut_on_tiles():
    nxg, nyg, buffer = S.VARYING
    t = terrain(nxg, nyg, seed=6)
    zb3, zt3 = S.varying_layers(t)
    nz = zb3.shape[1]
    tf, lt, buf = W.setup_linwinds(t.T.copy(), S.W3_DX, buffer)
    zb = [zb3[:, z, :].T.copy() for z in range(nz)]; zt = [zt3[:, z, :].T.copy() for z in range(nz)]
    ul, vl, *_ = W.build_lut(tf, lt, buf, zb, zt, lut_options(S.w3_options(buffer)), varying=True)
    for image in range(1, 5):
        d, opt, _ = w3_domain(nxg, nyg, buffer, 4, image, varying=(zb3, zt3), seed=6)
        try:
            got = (LW.lut_download(d, opt, 0), LW.lut_download(d, opt, 1))
            assert image == 1 or d.grid.ims > 1 or d.grid.jms > 1
        finally:
            d.close()
        for comp, (g, w) in enumerate(zip(got, tile_slices(d, ul, vl))):
            lut_close(g, w, f"space_varying_dz 4 images, image {image} comp {comp}")

"""The NSAS scheme on the device against its CPU restatement (tests/support/nsas_oracle.c) AND against the vectors of the compiled
reference (tests/golden/cu_nsas_*.npz): the six fixtures over their carried calls, icar_hip_cu_nsas alone on a sub-range of
its..ite, icar_hip_convect with fractions, hpbl uploaded against the default and read from YSU once YSU is initialised, the refusals,
and icar_hip_convection_init with 5, 1 and 0.  Every comparison: 0 differing bits."""
import os

import numpy as np
import pytest

import bmj_oracle as B
import nsas_oracle as N
import tiedtke_oracle as T
import ysu_oracle as Y
from icar_amd import convection, pbl
from icar_amd.capi import IcarHipError
from icar_amd.grid import grid_t
from util import equals_reference_vector, parity_record, single_image_domain

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES = N.TEND + N.OUT2
SENT = np.float32(-77.0)


@pytest.mark.parametrize("name", list(N.CASES))
def test_device_equals_restatement_and_reference_vectors(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = N.make_case(**N.CASES[name])
    assert float(z["input_fingerprint"]) == N.fingerprint(c)
    d = N.device_domain(c)
    A = N.state(c)
    tile = N.tile_of(c)
    for n in range(N.CALLS):
        N.run_oracle(c, A, n)                                                # (carries the state first)
        N.device_put(d, A)
        convection.cu_nsas(d, N.DT[n], *tile)
        got = N.device_state(d)
        for k in RES:
            assert N.bitdiff(N.owned(c, got[k]), N.owned(c, A[k])) == 0, f"{name}, call {n + 1}, {k}: differs from the restatement"
            assert equals_reference_vector(N.owned(c, got[k]), N.owned(c, z[f"call{n + 1}_{k}"])), f"{name}, call {n + 1}, {k}: differs from the compiled reference"
    parity_record("nsas", f"fixture/{name}", {k: {"bitdiff_cells": 0} for k in RES})
    d.close()


@pytest.fixture(scope="module")
def case():
    return N.make_case(nx=34, ny=12, nz=30, seed=31, dx=900.0)


def test_cu_nsas_alone_on_a_sub_range_touches_nothing_else(case):
    c = case
    ny, nz, nx = c["density"].shape
    d = N.device_domain(c)
    sub = (5, 29, 3, 9)
    for k in convection.CU_NAMES:
        convection.cu_set(d, k, np.full((ny, nz, nx) if k.startswith("tend") else (ny, nx), SENT, np.float32))
    for k in ("tend_qc", "tend_qi", "pratec", "hbot", "htop"):
        convection.nsas_set(d, k, np.full((ny, nz, nx) if k.startswith("tend") else (ny, nx), SENT, np.float32))
    names = ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature", "w_real", "u_mass", "v_mass", "sensible_heat", "latent_heat")
    before = {k: d.get(N.DEVICE_NAME.get(k, k)) for k in names}
    hp = convection.nsas_get(d, "hpbl")
    convection.cu_nsas(d, 60.0, *sub)
    A = N.state(c)
    N.cu_nsas(c, A, 60.0, sub)
    got = N.device_state(d)
    inside = np.zeros((ny, nx), bool); inside[sub[2] - 1:sub[3], sub[0] - 1:sub[1]] = True
    for k in RES:
        g, a = got[k], A[k]
        m = inside[:, None, :] & np.ones(g.shape, bool) if g.ndim == 3 else inside
        if g.ndim == 3:
            m = m.copy(); m[:, -1, :] = False
        assert N.bitdiff(g[m], a[m]) == 0, k
        assert (g[~m] == SENT).all(), f"{k} written outside its..ite, jts..jte"
    for k in N.TEND:
        assert (got[k][:, -1, :] == SENT).all(), f"{k}: the level kte belongs to nobody (cu_nsas runs on kts..kte-1)"
    for k in ("cldefi", "cutop", "cubot", "accumulated_convective_pcp"):
        assert (convection.cu_get(d, k) == SENT).all(), k
    for k, b in before.items():
        assert d.get(N.DEVICE_NAME.get(k, k)).tobytes() == b.tobytes(), k
    assert convection.nsas_get(d, "hpbl").tobytes() == hp.tobytes()
    dg = A["diag"][inside]
    assert (dg & N.D_DEEP_RAIN != 0).any() and (dg & N.D_SHALLOW != 0).any() and (dg & N.D_DXF1 != 0).all()
    d.close()


def test_convect_with_fractions(case):
    c = case
    fr = (0.5, 0.5, 0.0, 0.5)                                                # tendency_fraction 0.5 inherited, tend_th_fraction = 0
    d = N.device_domain(c, tendency_fraction=0.5, fractions=(-1.0, -1.0, 0.0, -1.0))
    A = N.state(c)
    A["accumulated_precipitation"] = np.zeros(c["xland"].shape, np.float64)
    A["accumulated_convective_pcp"] = np.zeros(c["xland"].shape, np.float32)
    g = d.grid
    tile = (g.its, g.ite, g.jts, g.jte)
    for n in range(2):
        if n:                                                                # diagnostic_update's temperature, on both sides
            A["temperature"] = (A["potential_temperature"] * c["exner"]).astype(np.float32)
            d.set("temperature", A["temperature"])
        convection.convect(d, d._cu_opt, N.DT[n])
        N.convect(c, A, N.DT[n], tile, 0.5, fr)
        got = N.device_state(d)
        for k in RES + ["potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "accumulated_precipitation", "accumulated_convective_pcp"]:
            assert N.bitdiff(got[k], A[k]) == 0, (n + 1, k, N.bitdiff(got[k], A[k]))
    assert N.bitdiff(A["potential_temperature"], c["potential_temperature"]) == 0 and (A["tend_th"] != 0).any(), "a fraction of 0 leaves the field alone"
    assert (A["cloud_water"] != c["cloud_water"]).any() and (A["raincv"] > 0).any()
    d.close()


def test_hpbl_uploaded_against_the_default(case):
    c = case
    d = single_image_domain(c)
    convection.convection_init(d, 4)                                         # dx from the domain; no boundary layer: hpbl = 1000
    d.fill("accumulated_precipitation", 0.0)
    assert (convection.nsas_get(d, "hpbl") == 1000.0).all()
    tile = N.tile_of(c)
    flat = np.full(c["hpbl"].shape, 1000.0, np.float32)
    hp = np.random.default_rng(5).uniform(300.0, 2500.0, c["hpbl"].shape).astype(np.float32)
    res = []
    for h in (flat, hp):
        convection.nsas_set(d, "hpbl", h)
        convection.cu_nsas(d, 60.0, *tile)
        A = N.state(c)
        N.cu_nsas(c, A, 60.0, tile, hpbl=h)
        got = N.device_state(d)
        for k in RES:
            assert N.bitdiff(N.owned(c, got[k]), N.owned(c, A[k])) == 0, k
        res.append(A["tend_th"].copy())
    assert N.bitdiff(res[0], res[1]) > 0, "the shallow scheme's mass flux reads hpbl (cu_nsas.f90:3125)"
    d.close()


def test_hpbl_is_read_from_ysu_once_ysu_is_initialised():
    cy = Y.make_case(nx=24, ny=10, nz=16, seed=3)
    c = N.make_case(nx=24, ny=10, nz=16, seed=3, dx=4000.0)
    d = Y.device_domain(cy)                                                   # pbl_init with kPBL_YSU
    d.load_case(c)                                                            # the NSAS case's fields on the same context
    d.dx = float(c["dx"])
    convection.convection_init(d, 4)
    d.fill("accumulated_precipitation", 0.0)
    assert (convection.nsas_get(d, "hpbl") == 0.0).all(), "with YSU, init_convection leaves hpbl alone (cu_driver.f90:180-186)"
    hp = np.random.default_rng(6).uniform(200.0, 3000.0, c["hpbl"].shape).astype(np.float32)
    pbl.ysu_set(d, "hpbl", hp)                                                # what ysu leaves in domain%hpbl
    tile = N.tile_of(c)
    convection.cu_nsas(d, 60.0, *tile)
    A = N.state(c)
    N.cu_nsas(c, A, 60.0, tile, hpbl=hp)
    got = N.device_state(d)
    for k in RES:
        assert N.bitdiff(N.owned(c, got[k]), N.owned(c, A[k])) == 0, k
    assert (N.owned(c, A["diag"]) & N.D_SHALLOW != 0).any()
    d.close()


def test_refusals(case):
    c = case
    d = single_image_domain(c)
    with pytest.raises(IcarHipError, match="not initialised"):
        convection.cu_nsas(d, 60.0, 2, 5, 2, 5)
    with pytest.raises(IcarHipError, match="kCU_NSAS.*not built.*icar_hip_convection_init"):
        convection.cu_init(d, 4)
    with pytest.raises(IcarHipError, match="kCU_NSAS.*not built.*icar_hip_convection_init"):
        convection.cu_configure(d, 4)
    for dx in (0.0, -1.0, float("nan")):
        with pytest.raises(IcarHipError, match="dx"):
            convection.convection_init(d, 4, dx=dx)
    with pytest.raises(IcarHipError, match="stochastic_cu"):
        convection.convection_init(d, 4, stochastic_cu=20.0)
    with pytest.raises(IcarHipError, match="not initialised"):
        convection.nsas_get(d, "hpbl")
    d.close()
    # levels: kts /= 1, too few, too many
    for nz, kts, word in ((2, 1, r"at least 3.*xlamue\(i,0\).*cu_nsas.f90:2456"), (130, 1, "at most 129"), (12, 2, "kts = 2")):
        cc = N.make_case(nx=6, ny=5, nz=nz, seed=3)
        g = grid_t().set_grid_dimensions(6, 5, nz, 1, 1)
        g.kts = kts
        dd = N.device_domain(cc, grid=g)
        convection.nsas_set(dd, "pratec", np.full((5, 6), SENT, np.float32))
        with pytest.raises(IcarHipError, match=word):
            convection.convect(dd, dd._cu_opt, 60.0)
        if kts == 2:
            with pytest.raises(IcarHipError, match="kts = 2"):
                convection.cu_nsas(dd, 60.0, 2, 5, 2, 4)
        assert (convection.nsas_get(dd, "pratec") == SENT).all(), "refused before any launch"
        dd.close()


def test_convection_init_5_and_1_equal_cu_init_and_0_is_never_configured():
    cb = B.make_case(nx=24, ny=10, nz=14, seed=3, rh_lo=0.6)
    a, b, never = single_image_domain(cb), single_image_domain(cb), single_image_domain(cb)
    convection.convection_init(a, 5, tendency_fraction=0.5, dx=0.0)          # dx is ignored
    convection.cu_init(b, 5, tendency_fraction=0.5)
    opt = B.options_of(cb); opt.cu_options.tendency_fraction = 0.5
    for d in (a, b):
        d.fill("accumulated_precipitation", 0.0)
        d._cu_key = (5, -9999.0, 0.5, 0.5, 0.5, 0.5, 0.5)
        convection.convect(d, opt, 40.0)
    for k in B.CU_ARRAYS:
        assert convection.cu_get(a, k).tobytes() == convection.cu_get(b, k).tobytes(), k
    for k in ("potential_temperature", "water_vapor", "cloud_water_mass", "cloud_ice_mass"):
        assert a.get(k).tobytes() == b.get(k).tobytes(), k
    assert (convection.cu_get(a, "raincv") > 0).any()
    # 0: convect returns at once, and a context on which nothing else was called is what a never-configured one is
    convection.convection_init(a, 0)
    before = {k: a.get(k) for k in ("potential_temperature", "water_vapor", "temperature")}
    off = B.options_of(cb); off.physics.convection = 0
    convection.convect(a, off, 40.0)
    for k, v in before.items():
        assert a.get(k).tobytes() == v.tobytes(), k
    convection.convection_init(never, 0)
    with pytest.raises(IcarHipError, match="not configured"):
        convection.cu_get(never, "raincv")
    for k in ("potential_temperature", "water_vapor", "temperature"):
        assert never.get(k).tobytes() == np.ascontiguousarray(cb[k], np.float32).tobytes(), k
    for d in (a, b, never):
        d.close()
    # 1: Tiedtke through the new entry point
    ct = T.make_case(nx=24, ny=10, nz=16, seed=3, depth_max=8000.0)
    a, b = single_image_domain(ct), single_image_domain(ct)
    convection.convection_init(a, 1, dx=-3.0)
    convection.cu_init(b, 1)
    for d in (a, b):
        d.fill("accumulated_precipitation", 0.0)
        convection.cu_tiedtke(d, 60.0, *T.tile_of(ct))
    sa, sb = T.device_state(a), T.device_state(b)
    for k in T.TEND + T.OUT2 + ["ktype"]:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    assert (sa["ktype"] == 3).any()
    for d in (a, b):
        d.close()

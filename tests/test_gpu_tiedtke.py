"""The Tiedtke scheme on the device against its CPU restatement (tests/support/tiedtke_oracle.c) AND against the vectors of the
compiled reference (tests/golden/cu_tiedtke_*.npz): the six fixtures over their carried calls, icar_hip_cu_tiedtke alone,
icar_hip_convect with fractions, the refusals, and icar_hip_cu_init with 5 and 0.  Every comparison: 0 differing bits."""
import os

import numpy as np
import pytest

import bmj_oracle as B
import tiedtke_oracle as T
from icar_amd import convection
from icar_amd.capi import IcarHipError
from icar_amd.grid import grid_t
from util import equals_reference_vector, parity_record, single_image_domain

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES = T.TEND + T.OUT2
SENT = np.float32(-77.0)


@pytest.mark.parametrize("name", list(T.CASES))
def test_device_equals_restatement_and_reference_vectors(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = T.make_case(**T.CASES[name])
    assert float(z["input_fingerprint"]) == T.fingerprint(c)
    d = T.device_domain(c)
    A = T.state(c)
    tile = T.tile_of(c)
    for n in range(T.CALLS):
        T.run_oracle(c, A, n)                                                # (carries the state first)
        T.device_put(d, A)
        convection.cu_tiedtke(d, T.DT[n], *tile)
        got = T.device_state(d)
        for k in RES + ["ktype"]:
            assert T.bitdiff(T.owned(c, got[k]), T.owned(c, A[k])) == 0, f"{name}, call {n + 1}, {k}: differs from the restatement"
        for k in RES:
            assert equals_reference_vector(T.owned(c, got[k]), T.owned(c, z[f"call{n + 1}_{k}"])), f"{name}, call {n + 1}, {k}: differs from the compiled reference"
    parity_record("tiedtke", f"fixture/{name}", {k: {"bitdiff_cells": 0} for k in RES})
    d.close()


@pytest.fixture(scope="module")
def case():
    return T.make_case(nx=34, ny=12, nz=30, seed=31)


def test_cu_tiedtke_alone_touches_nothing_else(case):
    c = case
    ny, nz, nx = c["density"].shape
    d = T.device_domain(c)
    sub = (5, 29, 3, 9)
    for k in convection.CU_NAMES:
        convection.cu_set(d, k, np.full((ny, nz, nx) if k.startswith("tend") else (ny, nx), SENT, np.float32))
    for k in ("tend_qc", "tend_qi", "pratec"):
        convection.tiedtke_set(d, k, np.full((ny, nz, nx) if k.startswith("tend") else (ny, nx), SENT, np.float32))
    convection.tiedtke_set(d, "ktype", np.full((ny, nx), -7, np.int32))
    before = {k: d.get(T.DEVICE_NAME.get(k, k)) for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "temperature", "w_real")}
    convection.cu_tiedtke(d, 60.0, *sub)
    A = T.state(c)
    T.cu_tiedtke(c, A, 60.0, sub)
    got = T.device_state(d)
    inside = np.zeros((ny, nx), bool); inside[sub[2] - 1:sub[3], sub[0] - 1:sub[1]] = True
    for k in RES + ["ktype"]:
        g, a = got[k], A[k]
        m = inside[:, None, :] & np.ones(g.shape, bool) if g.ndim == 3 else inside
        if g.ndim == 3:
            m = m.copy(); m[:, -1, :] = False
        assert T.bitdiff(g[m], a[m]) == 0, k
        assert (g[~m] == (-7 if k == "ktype" else SENT)).all(), f"{k} written outside its..ite, jts..jte"
    for k in T.TEND:
        assert (got[k][:, -1, :] == SENT).all(), f"{k}: the level kte belongs to nobody (CU_TIEDTKE runs on kts..kte-1)"
    for k in ("cldefi", "cutop", "cubot", "accumulated_convective_pcp"):
        assert (convection.cu_get(d, k) == SENT).all(), k
    for k, b in before.items():
        assert d.get(T.DEVICE_NAME.get(k, k)).tobytes() == b.tobytes(), k
    assert (A["ktype"] == 3).any()
    d.close()


def test_convect_with_fractions(case):
    c = case
    fr = (0.5, 0.5, 0.0, 0.5)                                                # tendency_fraction 0.5 inherited, tend_th_fraction = 0
    d = T.device_domain(c, tendency_fraction=0.5, fractions=(-1.0, -1.0, 0.0, -1.0))
    A = T.state(c)
    A["accumulated_precipitation"] = np.zeros(c["xland"].shape, np.float64)
    A["accumulated_convective_pcp"] = np.zeros(c["xland"].shape, np.float32)
    g = d.grid
    tile = (g.its, g.ite, g.jts, g.jte)
    for n in range(2):
        if n:                                                                # diagnostic_update's temperature, on both sides
            A["temperature"] = (A["potential_temperature"] * c["exner"]).astype(np.float32)
            d.set("temperature", A["temperature"])
        convection.convect(d, d._cu_opt, T.DT[n])
        T.convect(c, A, T.DT[n], tile, 0.5, fr)
        got = T.device_state(d)
        for k in RES + ["ktype", "potential_temperature", "water_vapor", "cloud_water", "cloud_ice", "accumulated_precipitation", "accumulated_convective_pcp"]:
            assert T.bitdiff(got[k], A[k]) == 0, (n + 1, k, T.bitdiff(got[k], A[k]))
    assert T.bitdiff(A["potential_temperature"], c["potential_temperature"]) == 0 and (A["tend_th"] != 0).any(), "a fraction of 0 leaves the field alone"
    assert (A["cloud_water"] != c["cloud_water"]).any() and (A["raincv"] > 0).any()
    d.close()


def test_refusals(case):
    c = case
    d = single_image_domain(c)
    with pytest.raises(IcarHipError, match="not initialised"):
        convection.cu_tiedtke(d, 60.0, 2, 5, 2, 5)
    for cu, word in ((4, "kCU_NSAS"), (2, "kCU_SIMPLE"), (3, "kCU_KAINFR")):
        with pytest.raises(IcarHipError, match=word):
            convection.cu_init(d, cu)
    with pytest.raises(IcarHipError, match="stochastic_cu"):
        convection.cu_init(d, 1, stochastic_cu=20.0)
    with pytest.raises(IcarHipError, match="NaN"):
        convection.cu_init(d, 1, tendency_fraction=float("nan"))
    d.znu = None
    with pytest.raises(IcarHipError, match="znu"):
        convection.cu_init(d, 1)
    with pytest.raises(IcarHipError, match="kCU_TIEDTKE.*icar_hip_cu_init"):
        convection.cu_configure(d, 1)
    d.close()
    # levels: kts /= 1, too few, too many
    for nz, kts, word in ((3, 1, r"at least 4.*PAPH\(JL,0\)"), (130, 1, "at most 129"), (12, 2, "kts = 2")):
        cc = T.make_case(nx=6, ny=5, nz=nz, seed=3)
        g = grid_t().set_grid_dimensions(6, 5, nz, 1, 1)
        g.kts = kts
        dd = T.device_domain(cc, grid=g)
        convection.tiedtke_set(dd, "pratec", np.full((5, 6), SENT, np.float32))
        with pytest.raises(IcarHipError, match=word):
            convection.convect(dd, dd._cu_opt, 60.0)
        if kts == 2:
            with pytest.raises(IcarHipError, match="kts = 2"):
                convection.cu_tiedtke(dd, 60.0, 2, 5, 2, 4)
        assert (convection.tiedtke_get(dd, "pratec") == SENT).all(), "refused before any launch"
        dd.close()


def test_cu_init_5_and_0_equal_cu_configure(case):
    cb = B.make_case(nx=24, ny=10, nz=14, seed=3, rh_lo=0.6)
    a, b, never = single_image_domain(cb), single_image_domain(cb), single_image_domain(cb)
    convection.cu_init(a, 5, tendency_fraction=0.5)
    convection.cu_configure(b, 5, tendency_fraction=0.5)
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
    # 0: convect returns at once, nothing is allocated, every field is what a context that was never configured holds
    convection.cu_init(a, 0)
    before = {k: a.get(k) for k in ("potential_temperature", "water_vapor", "temperature")}
    off = B.options_of(cb); off.physics.convection = 0
    convection.convect(a, off, 40.0)
    for k, v in before.items():
        assert a.get(k).tobytes() == v.tobytes(), k
    convection.cu_init(never, 0)
    with pytest.raises(IcarHipError, match="not configured"):
        convection.cu_get(never, "raincv")
    for k in ("potential_temperature", "water_vapor", "temperature"):
        assert never.get(k).tobytes() == np.ascontiguousarray(cb[k], np.float32).tobytes(), k
    for d in (a, b, never):
        d.close()

"""The convection slot on the device against its CPU restatement (tests/support/bmj_oracle.c) AND against the vectors of the compiled
reference (tests/golden/cu_bmj_*.npz): the six fixtures over their three carried calls, BMJINIT's tables as they sit in device
memory, each entry point alone, icar_hip_cu_reset.  Every comparison: 0 differing bits."""
import os

import numpy as np
import pytest

import bmj_oracle as B
from icar_amd import convection
from icar_amd.capi import IcarHipError
from util import bits_equal, equals_reference_vector, parity_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = B.STATE3 + B.STATE2
SENT = np.float32(-77.0)


def same(a, b):
    return B.bitdiff(a, b) == 0


@pytest.mark.parametrize("name", list(B.CASES))
def test_device_equals_restatement_and_reference_vectors(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = B.make_case(**B.CASES[name])
    assert float(z["input_fingerprint"]) == B.fingerprint(c)
    d = B.device_domain(c)
    A = B.state(c)
    for n in range(B.CALLS):
        B.device_call(d, c, n)
        B.run_oracle(c, A, n)
        got = B.device_state(d)
        for k in FIELDS + ["accumulated_precipitation"]:
            assert same(got[k], A[k]), f"{name}, call {n + 1}, {k}: {B.bitdiff(got[k], A[k])} cells differ from the restatement"
        for k in B.STATE2 + ["tend_th", "tend_qv"]:
            assert equals_reference_vector(got[k], z[f"call{n + 1}_{k}"]), f"{name}, call {n + 1}, {k}: differs from the compiled reference"
        assert same(got["accumulated_precipitation"], z[f"call{n + 1}_accumulated_precipitation"])
    for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice"):
        assert equals_reference_vector(got[k], z[f"call{B.CALLS}_{k}"]), (name, k)
    assert (got["raincv"] > 0).any() and (got["tend_th"] != 0).any()
    parity_record("cu", f"fixture/{name}", {k: {"bitdiff_cells": 0} for k in FIELDS})
    d.close()


@pytest.fixture(scope="module")
def case():
    return B.make_case(nx=34, ny=12, nz=20, seed=31, rh_lo=0.5)


def test_tables_on_the_device_equal_the_reference(case):
    d = B.device_domain(case)
    got = convection.cu_tables(d)
    z = np.load(os.path.join(GOLDEN, "cu_bmj_tables.npz"))
    mine = B.tables()
    for name, shape in B.TABLES:
        assert got[name].shape == shape
        assert equals_reference_vector(got[name], z[name]) and bits_equal(got[name], mine[name]), name
    d.close()


def test_cu_bmj_alone_touches_only_its_own_arrays(case):
    c = case
    d = B.device_domain(c)
    its, ite, jts, jte = B.tile_of(c)
    convection.cu_bmj(d, 40.0, its, ite, jts, jte)
    A = B.state(c)
    kind = B.drv(c, A, 40.0)
    got = B.device_state(d)
    for k in ("cldefi", "raincv", "cutop", "cubot", "tend_th", "tend_qv"):
        assert same(got[k], A[k]), (k, B.bitdiff(got[k], A[k]))
    for k in ("potential_temperature", "water_vapor", "cloud_water", "cloud_ice"):
        assert got[k].tobytes() == c[k].tobytes(), f"{k}: the scheme alone applies nothing"
    assert not got["accumulated_convective_pcp"].any() and not got["accumulated_precipitation"].any()
    sh = B.kinds_share(c, kind)
    assert sh["deep"] > 0.04 and sh["shallow"] > 0.02 and sh["none"] > 0.2, sh
    d.close()


def test_convect_is_zero_then_scheme_then_application(case):
    """icar_hip_convect against the three steps issued by hand: the zeroing over all i and k of the rows jts..jte (sentinels in the
    halo columns of the tendencies and of RAINCV go, those on the rows outside stay), the scheme, the application"""
    c = case
    ny, nz, nx = c["density"].shape
    d = B.device_domain(c)
    for k in ("tend_th", "tend_qv"):
        convection.cu_set(d, k, np.full((ny, nz, nx), SENT, np.float32))
    convection.cu_set(d, "raincv", np.full((ny, nx), SENT, np.float32))
    A = B.state(c)
    for k in ("tend_th", "tend_qv", "raincv"):
        A[k][...] = SENT
    B.device_call(d, c, 0)
    B.run_oracle(c, A, 0)
    got = B.device_state(d)
    for k in FIELDS + ["accumulated_precipitation"]:
        assert same(got[k], A[k]), (k, B.bitdiff(got[k], A[k]))
    its, ite, jts, jte = B.tile_of(c)
    assert (got["tend_th"][0] == SENT).all() and (got["raincv"][-1] == SENT).all(), "rows outside jts..jte are not zeroed"
    assert not got["tend_th"][jts - 1:jte, :, 0].any() and not got["raincv"][jts - 1:jte, -1].any(), "all i of memory on the rows of the tile"
    d.close()


def test_upload_download_round_trip_and_reset(case):
    c = case
    ny, nz, nx = c["density"].shape
    d = B.device_domain(c)
    rng = np.random.default_rng(5)
    for k in B.CU_ARRAYS:
        a = rng.random((ny, nz, nx) if k.startswith("tend") else (ny, nx)).astype(np.float32)
        convection.cu_set(d, k, a)
        assert convection.cu_get(d, k).tobytes() == a.tobytes(), k
    keep = {k: convection.cu_get(d, k) for k in B.CU_ARRAYS}
    convection.cu_reset(d)
    assert (convection.cu_get(d, "cldefi") == np.float32(B.AVGEFI())).all() and not convection.cu_get(d, "accumulated_convective_pcp").any()
    for k in ("raincv", "cutop", "cubot", "tend_th", "tend_qv"):
        assert convection.cu_get(d, k).tobytes() == keep[k].tobytes(), f"{k}: reset leaves it"
    with pytest.raises(IcarHipError, match="ICAR_CU_"):
        convection.cu_get(d, 9)
    d.close()


def test_convection_0_returns_at_once_and_unconfigured_entry_points_say_so(case):
    from util import single_image_domain
    d = single_image_domain(case)
    opt = B.options_of(case)
    opt.physics.convection = 0
    convection.convect(d, opt, 40.0)                                  # cu_driver.f90:264
    with pytest.raises(IcarHipError, match="not configured"):
        convection.cu_bmj(d, 40.0, 2, 3, 2, 3)
    with pytest.raises(IcarHipError, match="not configured"):
        convection.cu_get(d, "cldefi")
    d.close()

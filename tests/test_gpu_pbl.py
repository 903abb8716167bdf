"""HIP simple_pbl (row P1, icar_amd/csrc/pbl_simple.hip) against the CPU restatement of src/physics/pbl_simple.f90
(tests/support/pbl_oracle.c, itself pinned to the compiled reference by tests/test_pbl_oracle.py) and against the reference's
vectors directly: all six scalars after every one of three carried calls, 0 differing bits; the rows' sub-step counts; graupel,
the number concentrations and the ring outside its..jte untouched; sub-tiles; water-only, land-only and absent masks; and the
atomic row maximum's determinism."""
import hashlib
import os

import numpy as np
import pytest

import pbl_oracle as P
from icar_amd import pbl
from util import bits_equal, equals_reference_vector, parity_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNTOUCHED = {"graupel": "graupel_mass", "ice_number": "cloud_ice_number", "rain_number": "rain_number"}


def device_vs_restatement(c, label, calls=P.CALLS, tile=None, kts=1, kte=None, land=True, each_call=None):
    ny, nz, nx = c["z"].shape
    its, ite, jts, jte = tile or (2, nx - 1, 2, ny - 1)
    kte = nz if kte is None else kte
    d = P.device_domain(c, land=land)
    A = P.state(c)
    seen = set()
    for n in range(calls):
        pbl.simple_pbl(d, c["pbl_dt"], its, ite, jts, jte, kts, kte)
        nsub, _ = P.run_oracle(c, A, tile=(its, ite, jts, jte), kts=kts, kte=kte, land=land)
        got = P.device_state(d)
        for k in P.SCALARS:
            assert bits_equal(got[k], A[k]), f"{label}, call {n + 1}, {k}: {P.bitdiff(got[k], A[k])} of {A[k].size} cells differ"
        assert np.array_equal(pbl.nsubsteps(d)[jts - 1:jte], nsub[jts - 1:jte]), f"{label}, call {n + 1}: sub-step counts"
        seen |= set(nsub[jts - 1:jte].tolist())
        if each_call: each_call(n, got)
    ring = np.ones((ny, nz, nx), bool); ring[jts - 1:jte, kts - 1:min(kte, nz - 1) + 1, its - 1:ite] = False
    for k in P.SCALARS:
        assert np.array_equal(got[k][ring], c[k][ring]), f"{label}: {k} changed outside the tile"
    for k, m in UNTOUCHED.items():
        assert np.array_equal(d.get(m), c[k]), f"{label}: {k} is not mixed by the scheme"
    parity_record("pbl", label, {k: {"bitdiff_cells": 0, "cells": int(A[k].size)} for k in P.SCALARS} | {"nsubsteps": sorted(int(x) for x in seen)})
    d.close()
    return A, seen


@pytest.mark.parametrize("name", list(P.CASES))
def test_golden_cases_device_equals_restatement_and_reference_vectors(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = P.make_case(**P.CASES[name])
    assert float(z["input_fingerprint"]) == P.fingerprint(c)
    stored = []

    def direct(n, got):                 # the device against the compiled reference's vectors, no restatement in between
        for k in P.SCALARS:
            assert hashlib.sha256(got[k].tobytes()).hexdigest() == str(z[f"sha_call{n + 1}_{k}"]), (name, n + 1, k)
            if f"call{n + 1}_{k}" in z.files:
                assert equals_reference_vector(got[k], z[f"call{n + 1}_{k}"]), (name, n + 1, k)
                stored.append(k)

    A, seen = device_vs_restatement(c, f"golden/{name}", each_call=direct)
    assert len(stored) >= 2 and seen == set(z["nsubsteps"][:, 1:-1].ravel().tolist())


@pytest.fixture(scope="module")
def big_case():
    return P.make_case(512, 512, 40, seed=21, rough=10.0, dt=120.0)


def test_256x256x40_every_cell_three_calls():
    c = P.make_case(256, 256, 40, seed=20, rough=10.0, dt=120.0)
    A, seen = device_vs_restatement(c, "256x256x40")
    assert len(seen) >= 3 and 1 in seen, seen


def test_512x512x40_every_cell_three_calls(big_case):
    A, seen = device_vs_restatement(big_case, "512x512x40")
    assert len(seen) >= 3 and 1 in seen, seen
    assert all(np.isfinite(a).all() for a in A.values())


def test_512x512x40_same_bytes_five_times(big_case):
    """the row maximum is an atomic maximum of bit patterns: the order of arrival must not show"""
    c = big_case
    d = P.device_domain(c)
    ny, nz, nx = c["z"].shape
    first = None
    for n in range(5):
        for k in P.SCALARS:
            d.set(P.MEMBER[k], c[k])
        pbl.simple_pbl(d, c["pbl_dt"], 2, nx - 1, 2, ny - 1, 1, nz)
        got = {k: v.tobytes() for k, v in P.device_state(d).items()}
        got["nsub"] = pbl.nsubsteps(d).tobytes()
        if first is None: first = got
        assert got == first, f"run {n + 1} differs from run 1"
    parity_record("pbl", "512x512x40/five_identical_runs", {"runs": 5, "identical": True})
    d.close()


@pytest.mark.parametrize("tile,kts,kte", [((5, 17, 4, 9), 1, None), ((2, 29, 7, 7), 1, None), ((9, 9, 2, 19), 1, None), ((3, 28, 3, 18), 2, 33),
                                          ((1, 30, 1, 20), 1, None)])
def test_sub_tiles(tile, kts, kte):
    """its > 2, a one-row tile, a one-column tile, a shortened level range, and the whole memory extent"""
    c = P.make_case(**P.CASES["pbl_simple_b_30x20x40"])
    A, seen = device_vs_restatement(c, f"subtile/{tile}/k{kts}-{kte}", tile=tile, kts=kts, kte=kte)
    assert not np.array_equal(A["potential_temperature"], c["potential_temperature"])


@pytest.mark.parametrize("mask", ["water", "land", "absent"])
def test_masks(mask):
    c = P.make_case(**P.CASES["pbl_simple_e_20x12x24"])
    if mask != "absent":
        c["land_mask"] = np.full_like(c["land_mask"], 2 if mask == "water" else 1)
    A, seen = device_vs_restatement(c, f"mask/{mask}", land=mask != "absent")
    if mask == "absent":                # never uploaded == every cell is land
        c["land_mask"] = np.full_like(c["land_mask"], 1)
        B = P.state(c)
        for n in range(P.CALLS):
            P.run_oracle(c, B)
        for k in P.SCALARS:
            assert bits_equal(A[k], B[k]), k
    if mask == "water":
        assert seen == {1}, seen        # Kq / 1000 everywhere


def test_missing_member_is_named():
    from icar_amd.capi import IcarHipError
    c = P.make_case(**P.CASES["pbl_simple_c_calm_24x12x12"])
    d = P.device_domain({k: v for k, v in c.items() if k != "terrain"})
    with pytest.raises(IcarHipError, match="terrain"):
        pbl.simple_pbl(d, 30.0, 2, 23, 2, 11, 1, 12)
    d.close()


def test_surface_fields_are_not_forced_or_exchanged():
    import ctypes
    from icar_amd.capi import lib, IcarHipError
    from icar_amd import _fields as F
    c = P.make_case(**P.CASES["pbl_simple_c_calm_24x12x12"])
    d = P.device_domain(c)
    assert np.array_equal(d.get("land_mask"), c["land_mask"]) and d.get("land_mask").dtype == np.int32
    assert np.array_equal(d.get("terrain"), c["terrain"])
    for f in ("terrain", "land_mask"):
        with pytest.raises(IcarHipError):
            d.set_dqdt(f, np.zeros(d.shape(d.fid(f)), np.float32))
        with pytest.raises(IcarHipError):
            d.apply_forcing(1.0, [(f, False)])
        ids = (ctypes.c_int * 1)(d.fid(f))
        buf = d.new_buffer(4096)                # (halo_send / halo_retrieve pack through the same check once a transport is attached)
        assert lib().icar_hip_halo_pack(d.ctx, 0, 1, ids, 1, ctypes.c_void_p(buf.data_ptr())) != 0
        assert b"exchangeable" in lib().icar_hip_last_error()
    d.close()

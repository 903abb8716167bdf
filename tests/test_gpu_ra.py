"""HIP ra_simple (row R1, icar_amd/csrc/ra_simple.hip) against the CPU restatement of src/physics/ra_simple.f90
(tests/support/ra_oracle.c, itself pinned to the compiled reference by tests/test_ra_oracle.py) and against the reference's vectors
directly: theta, swdown, lwdown and cloud_cover on the tile after every one of three carried calls (dt growing, the clock
advancing), 0 differing bits; cloud_cover's 5e-8 columns outside its:ite; everything else untouched; F_runlw = .false.; a
latitude uploaded again; a missing member."""
import hashlib
import os

import numpy as np
import pytest

import ra_oracle as R
from util import bits_equal, equals_reference_vector, parity_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def compare(got, A, c, label, tile=None):
    m, rows = R.tile_mask(c, tile)
    assert bits_equal(got["potential_temperature"], A["potential_temperature"]), f"{label}: theta, {R.bitdiff(got['potential_temperature'], A['potential_temperature'])} cells differ"
    # (the restatement leaves swdown / lwdown outside its:ite untouched like the device: the whole arrays are compared)
    for k in R.OUTPUTS[1:]:
        assert bits_equal(got[k], A[k]), f"{label}: {k}, {R.bitdiff(got[k], A[k])} of {A[k].size} cells differ"
    assert (got["cloud_fraction"][rows & ~m] == np.float32(5e-8)).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_golden_cases_device_equals_restatement_and_reference_vectors(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = R.make_case(**R.CASES[name])
    assert float(z["input_fingerprint"]) == R.fingerprint(c)
    m, rows = R.tile_mask(c)
    d = R.device_domain(c)
    A = R.state(c)
    for n in range(R.CALLS):
        R.device_call(d, c, n)
        R.run_oracle(c, A, n)
        got = R.device_state(d)
        compare(got, A, c, f"{name}, call {n + 1}")
        # the device against the compiled reference's vectors, no restatement in between
        assert hashlib.sha256(got["potential_temperature"].tobytes()).hexdigest() == str(z[f"sha_call{n + 1}_potential_temperature"]), (name, n + 1)
        for k in R.OUTPUTS[1:]:
            assert hashlib.sha256(np.ascontiguousarray(got[k][m]).tobytes()).hexdigest() == str(z[f"sha_call{n + 1}_{k}"]), (name, n + 1, k)
            keep = m | rows if k == "cloud_fraction" else m
            assert equals_reference_vector(got[k][keep], z[f"call{n + 1}_{k}"][keep]), (name, n + 1, k)
        assert hashlib.sha256(np.ascontiguousarray(got["cloud_fraction"][rows]).tobytes()).hexdigest() == str(z[f"sha_call{n + 1}_cloud_fraction_rows"])
    if not c["runlw"]:
        assert np.array_equal(got["potential_temperature"], c["potential_temperature"]) and (got["longwave"] == np.float32(R.SENTINEL)).all()
    for k in R.INPUTS[1:] + ["latitude", "longitude"]:
        assert np.array_equal(d.get({"cloud_water": "cloud_water_mass", "snow": "snow_mass", "cloud_ice": "cloud_ice_mass", "graupel": "graupel_mass", "rain": "rain_mass"}.get(k, k)), c[k]), f"{k} is an input"
    parity_record("ra", f"golden/{name}", {k: {"bitdiff_cells": 0, "cells": int(A[k].size)} for k in R.OUTPUTS})
    d.close()


def test_runlw_false_leaves_theta_and_lwdown_untouched():
    c = R.make_case(**R.CASES["ra_simple_a_40x36x20"])
    d = R.device_domain(c)
    A = R.state(c)
    R.device_call(d, c, 0, runlw=False)
    R.run_oracle(c, A, 0, runlw=False)
    got = R.device_state(d)
    compare(got, A, c, "runlw = false")
    assert got["potential_temperature"].tobytes() == c["potential_temperature"].tobytes()
    assert (got["longwave"] == np.float32(R.SENTINEL)).all()
    m, _ = R.tile_mask(c)
    assert (got["shortwave"][m] >= 0).all() and (got["shortwave"][m] > 0).any()
    R.device_call(d, c, 1, runlw=True)                      # and the same context with the longwave on
    R.run_oracle(c, A, 1, runlw=True)
    compare(R.device_state(d), A, c, "runlw = true after false")
    d.close()


def test_latitude_uploaded_again_is_used():
    c = R.make_case(**R.CASES["ra_simple_b_noleap_26x14x5"])
    d = R.device_domain(c)
    A = R.state(c)
    R.device_call(d, c, 0); R.run_oracle(c, A, 0)
    c2 = dict(c); c2["latitude"] = np.ascontiguousarray(-c["latitude"][:, ::-1])
    d.set("latitude", c2["latitude"])
    R.device_call(d, c2, 1); R.run_oracle(c2, A, 1)
    compare(R.device_state(d), A, c2, "latitude uploaded again")
    d.close()


def test_missing_member_and_missing_calendar_are_named():
    from icar_amd.capi import IcarHipError
    from icar_amd import radiation
    from util import single_image_domain
    c = R.make_case(**R.CASES["ra_simple_b_noleap_26x14x5"])
    d = single_image_domain({k: v for k, v in c.items() if k != "longitude"})
    with pytest.raises(IcarHipError, match="calendar"):
        radiation.ra_simple(d, 30.0, 2, 25, 2, 13, 1, 5)
    radiation.rad_calendar(d, 0, 0.0, 365, 365)
    with pytest.raises(IcarHipError, match="longitude"):
        radiation.ra_simple(d, 30.0, 2, 25, 2, 13, 1, 5)
    assert d.get("potential_temperature").tobytes() == c["potential_temperature"].tobytes()
    d.close()

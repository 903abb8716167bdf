"""The device's REAL(4) sin / cos / asin (icar_amd/csrc/glibc_flt32_trig.h: the C library's sinf / cosf / asinf restated) against
the HOST's libm, bit for bit: a stratified sample of 2^24 bit patterns per function over the whole REAL(4) line (every 256th,
with a per-function offset: every exponent, both signs, denormals, infinities and NaNs, the large-argument reduction) and the
arguments the radiation scheme produces.  The same header is checked on the CPU against every one of the 2^32 arguments
(tests/test_glibc_flt32_trig_host.py); this is the run on the device.  The host values come from tests/support/ra_oracle.c."""
import ctypes
import os
import sys

import numpy as np
import pytest

import ra_oracle as R
from util import parity_record

pytestmark = pytest.mark.gpu
FUNCS = {"sinf": 0, "cosf": 1, "asinf": 2}


@pytest.fixture(scope="module")
def trig():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "support"))
    import build_trig_probe
    return build_trig_probe.lib()


def device(trig, name, x):
    x = np.ascontiguousarray(x, np.float32); y = np.empty_like(x)
    rc = trig.icar_trig_probe(FUNCS[name], x.size, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, f"trig probe: HIP error {rc}"
    return y


def differing(got, want):
    return ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))


@pytest.mark.parametrize("name", list(FUNCS))
def test_stratified_sample_of_the_real4_line(trig, name):
    off = (37 * (FUNCS[name] + 10)) % 256
    x = (np.arange(1 << 24, dtype=np.uint64) * 256 + off).astype(np.uint32).view(np.float32)
    got, want = device(trig, name, x), R.libm(name, x)
    bad = differing(got, want)
    parity_record("trig_math", f"device {name} vs the host libm on a stratified 2^24 sample of the REAL(4) arguments", {"n": int(x.size), "differ": int(bad.sum())})
    assert not bad.any(), f"{name}: {int(bad.sum())} of {x.size} differ from libm, first x = {x[bad][0]!r}: {got[bad][0]!r} vs {want[bad][0]!r}"


def test_the_arguments_the_scheme_produces(trig):
    rng = np.random.default_rng(12)
    f = np.float32
    n = 1 << 20
    pi = f(3.1415927)
    doy = rng.uniform(-1.0, 367.0, n).astype(f)
    args = {"sinf": [rng.uniform(-90, 90, n).astype(f) / f(360) * f(2) * pi, rng.uniform(-0.4091, 0.4091, n).astype(f), rng.uniform(0, 1.5707964, n).astype(f),
                     np.array([0.0, -0.0, 1.5707964, -1.5707964, 0.7853982, 0.78539816, 120.0, 119.99999, 1e-5, 2.4e-4], f)],
            "cosf": [rng.uniform(-90, 90, n).astype(f) / f(360) * f(2) * pi, f(2) * pi / f(365) * (doy + f(10)), f(2) * pi * np.fmod(doy + f(0.5), f(1)),
                     np.fmod(doy / f(365), f(1)) * f(2) * pi, np.array([0.0, 6.2831855, 6.283185, 3.1415927, 1.5707964, -1.5707964], f)],
            "asinf": [rng.uniform(-1, 1, n).astype(f), (f(1) - rng.uniform(0, 1e-5, n).astype(f)), -(f(1) - rng.uniform(0, 1e-5, n).astype(f)),
                      np.array([1.0, -1.0, 0.5, -0.5, 0.975, 0.97500002, 0.0, -0.0, 7.4e-9, 0.99999994], f)]}
    stats = {}
    for name, xs in args.items():
        x = np.concatenate(xs)
        got, want = device(trig, name, x), R.libm(name, x)
        bad = differing(got, want)
        stats[name] = {"n": int(x.size), "differ": int(bad.sum())}
        assert not bad.any(), f"{name}: {int(bad.sum())} of {x.size} differ from libm, first x = {x[bad][0]!r}: {got[bad][0]!r} vs {want[bad][0]!r}"
    parity_record("trig_math", "device sinf / cosf / asinf vs the host libm on the radiation scheme's arguments", stats)

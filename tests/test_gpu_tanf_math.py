"""The device's REAL(4) tan (icar_amd/csrc/glibc_flt32_tan.h: the C library's tanf restated) against the HOST's libm, bit for
bit: a stratified sample of 2^24 bit patterns over the whole REAL(4) line (every 256th, from an offset: every exponent, both
signs, denormals, infinities and NaNs, the large-argument reduction) and the arguments the Tiedtke scheme produces
(cu_tiedtke.f90's CUENTR_NEW: TAN(3.1415 * r * 0.5), r in [0, 1]).  The same header is checked on the CPU against every one of
the 2^32 arguments (tests/test_glibc_flt32_tanf_host.py); this is the run on the device.  The host values come from
tests/support/tanf_host.c."""
import ctypes
import os
import sys

import numpy as np
import pytest

from util import parity_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "support"))
    import build_tanf_probe
    return build_tanf_probe.lib(), build_tanf_probe.host_lib()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def both(probe, x):
    dev, host = probe
    x = np.ascontiguousarray(x, np.float32); got = np.empty_like(x); want = np.empty_like(x)
    rc = dev.icar_tanf_probe(x.size, _p(x), _p(got))
    assert rc == 0, f"tanf probe: HIP error {rc}"
    host.icar_tanf_host(x.size, _p(x), _p(want))
    return got, want


def differing(got, want):
    return ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))


def test_stratified_sample_of_the_real4_line(probe):
    x = (np.arange(1 << 24, dtype=np.uint64) * 256 + 225).astype(np.uint32).view(np.float32)
    got, want = both(probe, x)
    bad = differing(got, want)
    parity_record("tanf_math", "device tanf vs the host libm on a stratified 2^24 sample of the REAL(4) arguments", {"n": int(x.size), "differ": int(bad.sum())})
    assert not bad.any(), f"tanf: {int(bad.sum())} of {x.size} differ from libm, first x = {x[bad][0]!r}: {got[bad][0]!r} vs {want[bad][0]!r}"


def test_the_arguments_the_scheme_produces(probe):
    rng = np.random.default_rng(17)
    f = np.float32
    n = 1 << 20
    # arg = 3.1415 * (zzmzk / ztmzk) * 0.5 in REAL(4), left to right; the ratio is a quotient of two heights with 0 <= zzmzk <= ztmzk
    top = rng.uniform(50.0, 15000.0, n).astype(f)
    r = [rng.uniform(0.0, 1.0, n).astype(f), (rng.uniform(0.0, 1.0, n).astype(f) * top) / top, f(1) - rng.uniform(0, 1e-5, n).astype(f),
         rng.uniform(0, 1e-4, n).astype(f), np.linspace(0.0, 1.0, 4097).astype(f), np.array([0.0, 1.0, 0.5, 0.42935, 0.42936, 0.99999994, 7.8e-5, 1e-30], f)]
    x = np.concatenate([f(3.1415) * q * f(0.5) for q in r])
    # ... and the neighbourhood of every threshold of the function: pi/4 (no reduction below), 0.6744 (tan from pi/4 - x),
    # 2^-13 (tan(x) = x), pi/2 (the reduced argument's head and tail), 120 (the large-argument reduction)
    edges = np.array([0x3f490fda, 0x3f2ca140, 0x39000000, 0x3fc90fdb, 0x42f00000], np.uint32)
    near = (edges[:, None].astype(np.int64) + np.arange(-64, 65)[None, :]).astype(np.uint32).ravel()
    x = np.concatenate([x, near.view(f), (near | np.uint32(0x80000000)).view(f)])
    got, want = both(probe, x)
    bad = differing(got, want)
    parity_record("tanf_math", "device tanf vs the host libm on the Tiedtke scheme's arguments and the function's thresholds", {"n": int(x.size), "differ": int(bad.sum())})
    assert not bad.any(), f"tanf: {int(bad.sum())} of {x.size} differ from libm, first x = {x[bad][0]!r}: {got[bad][0]!r} vs {want[bad][0]!r}"

"""Builds tests/support/libicar_tanf_probe.so (tanf_probe.hip: the device's tanf on arrays) with the product's own compile flags,
and tests/support/libtanf_host.so (tanf_host.c: the host C library's tanf on arrays).  TEST INFRASTRUCTURE: called by
__graft_entry__.build() (so that the files travel to the GPU box with the other built libraries) and by
tests/test_gpu_tanf_math.py.  Cross-compiles without a GPU."""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libicar_tanf_probe.so")
HOST_LIB = os.path.join(HERE, "libtanf_host.so")


def _stale(target, deps, force):
    return force or not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def build(force=False):
    sys.path.insert(0, ROOT)
    from icar_amd import build as B
    src = os.path.join(HERE, "tanf_probe.hip")
    if _stale(LIB, [src] + [os.path.join(B.CSRC, h) for h in ("glibc_flt32.h", "glibc_flt32_trig.h", "glibc_flt32_tan.h")], force):
        subprocess.check_call([B.HIPCC] + B.FLAGS + ["-I" + B.CSRC, "-shared", src, "-o", LIB])
    host = os.path.join(HERE, "tanf_host.c")
    if _stale(HOST_LIB, [host], force):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", host, "-o", HOST_LIB, "-lm"])
    return LIB


def lib():
    L = ctypes.CDLL(build())
    L.icar_tanf_probe.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    return L


def host_lib():
    build()
    L = ctypes.CDLL(HOST_LIB)
    L.icar_tanf_host.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.icar_tanf_host.restype = None
    return L


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))

"""Builds tests/support/libicar_trig_probe.so (trig_probe.hip: the device's sinf / cosf / asinf on arrays) with the product's own
compile flags.  TEST INFRASTRUCTURE: called by __graft_entry__.build() (so that the file travels to the GPU box with the other
built libraries) and by tests/test_gpu_trig_math.py.  Cross-compiles without a GPU."""
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libicar_trig_probe.so")


def build(force=False):
    sys.path.insert(0, ROOT)
    from icar_amd import build as B
    src = os.path.join(HERE, "trig_probe.hip")
    deps = [src, os.path.join(B.CSRC, "glibc_flt32.h"), os.path.join(B.CSRC, "glibc_flt32_trig.h")]
    if force or not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call([B.HIPCC] + B.FLAGS + ["-I" + B.CSRC, "-shared", src, "-o", LIB])
    return LIB


def lib():
    L = ctypes.CDLL(build())
    L.icar_trig_probe.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    return L


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))

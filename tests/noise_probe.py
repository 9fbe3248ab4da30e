"""Builds and binds tests/probe/noise_probe.hip (test helper): the device functions of csrc/noise_spec.h behind C entry points.

The probe is compiled with the product's compiler and exactly its flags (build.HIPCC_FLAGS, -I csrc) into the package's
lib/ directory, beside the product's library: git-ignored, and found already built by whoever runs the tree after a CPU
build.  Built on first use and when older than its sources, under the file lock build.py uses.
"""
import ctypes as C
import fcntl
import os

import numpy as np

from ccv_mppi_path_tracker_amd import build

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "probe", "noise_probe.hip")
DEPS = [SOURCE, os.path.join(build.CSRC, "noise_spec.h")]
LIB = os.path.join(build.LIBDIR, "libnoise_probe.so")
PHILOX_FORMS, BOX_MULLER_FORMS = (0, 3, 4, 5), (0, 6, 8, 10)


def stale():
    return not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS)


def command(out):
    return [build.hipcc()] + build.HIPCC_FLAGS + ["-I", build.CSRC, "-shared", "-o", out, SOURCE]


def build_probe(force=False):
    if not force and not stale():
        return LIB
    os.makedirs(build.LIBDIR, exist_ok=True)
    with open(os.path.join(build.LIBDIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or stale():                       # (another process may have built it while this one waited)
                tmp = LIB + ".tmp%d" % os.getpid()
                build._run(command(tmp), False)
                os.replace(tmp, LIB)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build_probe())
        u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        L.probe_philox.argtypes = [C.c_int, C.c_size_t, u32p, u32p, u32p]
        L.probe_box_muller.argtypes = [C.c_int, C.c_size_t, u32p, u32p, fp, fp]
        L.probe_sqrt.argtypes = [C.c_size_t, fp, fp, fp]
        _lib = L
    return _lib


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s: HIP error %d" % (what, rc))


def philox(form, ctr, key):
    """counters [n][4] under one key [2] -> uint32 [n][4] by philox4x32_10 (form 0) or philox4x32_10_n<form>"""
    ctr, key = _u32(ctr).reshape(-1, 4), _u32(key).reshape(2)
    out = np.empty_like(ctr)
    _ok(lib().probe_philox(form, ctr.shape[0], _p(ctr, C.c_uint32), _p(key, C.c_uint32), _p(out, C.c_uint32)), "probe_philox")
    return out


def box_muller(form, a, b):
    """words a, b [n] -> (z0, z1) float32 [n] by box_muller_f32 (form 0) or box_muller_f32_n<form>"""
    a, b = _u32(a).ravel(), _u32(b).ravel()
    assert a.shape == b.shape
    z0, z1 = np.empty(a.size, dtype=np.float32), np.empty(a.size, dtype=np.float32)
    _ok(lib().probe_box_muller(form, a.size, _p(a, C.c_uint32), _p(b, C.c_uint32), _p(z0, C.c_float), _p(z1, C.c_float)),
        "probe_box_muller")
    return z0, z1


def sqrt(x):
    """x float32 [n] -> (sqrt_cr_radius(x), __builtin_sqrtf(x))"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    s_cr, s_b = np.empty_like(x), np.empty_like(x)
    _ok(lib().probe_sqrt(x.size, _p(x, C.c_float), _p(s_cr, C.c_float), _p(s_b, C.c_float)), "probe_sqrt")
    return s_cr, s_b

"""Builds and binds tests/probe/select_probe.hip (test helper): select_lowest() of csrc/mppi_select.h behind a C entry point.

Built as tests/noise_probe.py builds its probe: the product's compiler and exactly its flags (build.HIPCC_FLAGS, -I csrc),
into the package's lib/ directory beside the product's library, on first use and when older than its sources, under the file
lock build.py uses.
"""
import ctypes as C
import fcntl
import os

import numpy as np

from ccv_mppi_path_tracker_amd import build

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "probe", "select_probe.hip")
DEPS = [SOURCE, os.path.join(build.CSRC, "mppi_select.h")]
LIB = os.path.join(build.LIBDIR, "libselect_probe.so")


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
        L.probe_select.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def lowest(segments, k, n):
    """segments float64 [S][pitch], of which columns 0 .. k - 1 take part -> (idx int32 [S][n], key uint64 [S][n]) by
    select_lowest(), one workgroup per segment"""
    seg = np.ascontiguousarray(segments, dtype=np.float64)
    assert seg.ndim == 2
    idx, key = np.empty((seg.shape[0], n), dtype=np.int32), np.empty((seg.shape[0], n), dtype=np.uint64)
    rc = lib().probe_select(seg.shape[0], seg.shape[1], int(k), int(n), seg.ctypes.data_as(C.POINTER(C.c_double)),
                            idx.ctypes.data_as(C.POINTER(C.c_int32)), key.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise RuntimeError("probe_select: HIP error %d" % rc)
    return idx, key

"""Builds and binds tests/probe/top_probe.hip (test helper): top_weights() and top_order_pairs() of csrc/mppi_top_weights.h
behind a C entry point.

Built as tests/select_probe.py builds its probe: the product's compiler and exactly its flags (build.HIPCC_FLAGS, -I csrc),
into the package's lib/ directory beside the product's library, on first use and when older than its sources, under the file
lock build.py uses.
"""
import ctypes as C
import fcntl
import os

import numpy as np

from ccv_mppi_path_tracker_amd import build

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "probe", "top_probe.hip")
HEADER = os.path.join(build.CSRC, "mppi_top_weights.h")
DEPS = [SOURCE, HEADER]
LIB = os.path.join(build.LIBDIR, "libtop_probe.so")


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
        L.probe_top.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def top(vectors, k, n):
    """vectors float64 [S][pitch], of which columns 0 .. k - 1 take part, one workgroup per vector ->
    (raw_idx int32 [S][n], raw_bits uint64 [S][n], ord_idx, ord_bits): the kernel's own layout, and the same after the host
    ordering; the weights as their bit patterns"""
    w = np.ascontiguousarray(vectors, dtype=np.float64)
    assert w.ndim == 2
    S = w.shape[0]
    raw_idx, raw_bits = np.empty((S, n), dtype=np.int32), np.empty((S, n), dtype=np.uint64)
    ord_idx, ord_bits = np.empty((S, n), dtype=np.int32), np.empty((S, n), dtype=np.uint64)
    i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    rc = lib().probe_top(S, w.shape[1], int(k), int(n), w.ctypes.data_as(C.POINTER(C.c_double)), raw_idx.ctypes.data_as(i32),
                         raw_bits.ctypes.data_as(u64), ord_idx.ctypes.data_as(i32), ord_bits.ctypes.data_as(u64))
    if rc != 0:
        raise RuntimeError("probe_top: HIP error %d" % rc)
    return raw_idx, raw_bits, ord_idx, ord_bits

"""CPU checks of the batch handles' disc obstacles (ccv_mppi_batch_set_obstacles / _get_obstacles, CCV_MPPI_MAX_OBSTACLES,
CCV_MPPI_BATCH_KERNEL_OBST): declared in the public header, exported by the library, mirrored by the ctypes table and the
Python class, the [B][max_n][3] marshalling, a null handle refused, and the header still C99."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
OBST = {"ccv_mppi_batch_set_obstacles", "ccv_mppi_batch_get_obstacles"}


def test_obstacle_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert OBST <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in OBST:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES
        assert capi.SIGNATURES[name][1][3] is C.c_int32
    assert capi.BATCH_KERNEL_OBST == int(re.search(r"#define CCV_MPPI_BATCH_KERNEL_OBST (\d+)", text).group(1)) == 128
    assert capi.MAX_OBSTACLES == int(re.search(r"#define CCV_MPPI_MAX_OBSTACLES (\d+)", text).group(1)) == 32
    # the OBST bit is distinct from the kernel codes and the other mode bits
    assert capi.BATCH_KERNEL_OBST & (capi.BATCH_KERNEL_ONE_WAVE | capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE |
                                     capi.BATCH_KERNEL_VARIED | capi.BATCH_KERNEL_SHIFT) == 0


def test_obstacle_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_obst.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, const double*, const int32_t*, int32_t, const double*);\n'
        'typedef int (*get_fn)(ccv_mppi_batch*, double*, int32_t*, int32_t, double*);\n'
        'int main(void){set_fn a = ccv_mppi_batch_set_obstacles; get_fn b = ccv_mppi_batch_get_obstacles;\n'
        'return (a && b && CCV_MPPI_BATCH_KERNEL_OBST > CCV_MPPI_BATCH_KERNEL_SHIFT && CCV_MPPI_MAX_OBSTACLES == 32) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_obst.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    xyr, n, w = np.zeros((1, 1, 3)), np.zeros(1, dtype=np.int32), np.zeros(1)
    ip = n.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ccv_mppi_batch_set_obstacles(None, capi.dptr(xyr), ip, 1, capi.dptr(w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_obstacles(None, None, None, 0, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_obstacles(None, capi.dptr(xyr), ip, 1, capi.dptr(w)) == capi.ERR_INVALID_ARG


def test_the_python_class_offers_the_term():
    assert callable(BatchController.set_obstacles) and callable(BatchController.get_obstacles)


def test_pack_obstacles_marshals_rows_counts_and_weights():
    discs = [np.array([[1.0, 2.0, 0.5], [3.0, 4.0, 0.25], [5.0, 6.0, 0.125]]), [], [(7.0, 8.0, 1.0)], None]
    xyr, n, max_n, w = batch.pack_obstacles(discs, [1.0, 2.0, 3.0, 4.0], 4)
    assert xyr.shape == (4, 3, 3) and xyr.dtype == np.float64 and xyr.flags["C_CONTIGUOUS"]
    assert n.dtype == np.int32 and n.tolist() == [3, 0, 1, 0] and max_n == 3
    np.testing.assert_array_equal(xyr[0], discs[0])
    np.testing.assert_array_equal(xyr[2, 0], (7.0, 8.0, 1.0))
    assert not xyr[1].any() and not xyr[2, 1:].any() and not xyr[3].any()   # rows past an instance's count: zero
    np.testing.assert_array_equal(w, [1.0, 2.0, 3.0, 4.0])
    # one weight for all; no disc anywhere: max_n = 0 (the library reads that as "off")
    xyr, n, max_n, w = batch.pack_obstacles([[], []], 5.0, 2)
    assert xyr.shape == (2, 0, 3) and max_n == 0 and w.tolist() == [5.0, 5.0]
    # instance (b, j) sits at flat offset (b * max_n + j) * 3, as the header says
    xyr, n, max_n, _ = batch.pack_obstacles([[(1, 2, 3)], [(4, 5, 6), (7, 8, 9)]], 0.0, 2)
    assert xyr.ravel()[(1 * max_n + 1) * 3:(1 * max_n + 1) * 3 + 3].tolist() == [7.0, 8.0, 9.0]


def test_pack_obstacles_refuses_bad_shapes():
    with pytest.raises(ValueError):
        batch.pack_obstacles([[]], 1.0, 2)                                   # one array for two instances
    with pytest.raises(ValueError):
        batch.pack_obstacles([[(1.0, 2.0)]], 1.0, 1)                         # not triples
    with pytest.raises(ValueError):
        batch.pack_obstacles([np.zeros((capi.MAX_OBSTACLES + 1, 3))], 1.0, 1)
    with pytest.raises(ValueError):
        batch.pack_obstacles([[]], [1.0, 2.0], 1)                            # two weights for one instance

"""CPU checks of the batch handles' occupancy grids (ccv_mppi_batch_set_grids / _get_grids / _read_grid_cells, struct
ccv_mppi_grid, CCV_MPPI_BATCH_KERNEL_GRID): declared in the public header, exported by the library, mirrored by the ctypes table
and the Python class, the struct's layout against capi.Grid through a compiled C program, the header still C99, a null handle
refused.  (The refusals that need a handle: tests/test_gpu_batch_grid.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
GRID = {"ccv_mppi_batch_set_grids", "ccv_mppi_batch_get_grids", "ccv_mppi_batch_read_grid_cells"}
FIELDS = ["origin_x", "origin_y", "resolution", "outside", "nx", "ny", "cells"]


def test_grid_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert GRID <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    assert not any("_resident_" in name for name in GRID)
    lib = C.CDLL(build.build())
    for name in GRID:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES and capi.SIGNATURES[name][0] is C.c_int
    assert capi.SIGNATURES["ccv_mppi_batch_set_grids"][1][1:] == [C.POINTER(capi.Grid), C.c_int32, C.POINTER(C.c_int32),
                                                                   C.POINTER(C.c_double)]
    assert capi.SIGNATURES["ccv_mppi_batch_read_grid_cells"][1][1:] == [C.c_int32, C.POINTER(C.c_float)]


def test_the_grid_flag_is_512_and_disjoint_from_the_others():
    text = open(HEADER).read()
    assert capi.BATCH_KERNEL_GRID == int(re.search(r"#define CCV_MPPI_BATCH_KERNEL_GRID (\d+)", text).group(1)) == 512
    others = (capi.BATCH_KERNEL_PLAIN | capi.BATCH_KERNEL_ONE_WAVE | capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE |
              capi.BATCH_KERNEL_VARIED | capi.BATCH_KERNEL_SHIFT | capi.BATCH_KERNEL_OBST | capi.BATCH_KERNEL_MOVING)
    assert capi.BATCH_KERNEL_GRID & others == 0
    defined = {int(v) for v in re.findall(r"#define CCV_MPPI_BATCH_KERNEL_[A-Z_]+ (\d+)", text)}
    assert len(defined) == len(re.findall(r"#define CCV_MPPI_BATCH_KERNEL_[A-Z_]+ (\d+)", text))


def test_the_struct_layout_is_the_ctypes_mirror(tmp_path):
    src = tmp_path / "grid_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ccv_mppi.h"\n'
                   'int main(void){printf("%zu", sizeof(ccv_mppi_grid));\n' +
                   "".join('printf(" %%zu", offsetof(ccv_mppi_grid, %s));\n' % f for f in FIELDS) + 'return 0;}\n')
    exe = tmp_path / "grid_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert [f for f, _ in capi.Grid._fields_] == FIELDS
    assert got == [C.sizeof(capi.Grid)] + [getattr(capi.Grid, f).offset for f in FIELDS]


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_grid.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, const ccv_mppi_grid*, int32_t, const int32_t*, const double*);\n'
        'typedef int (*get_fn)(ccv_mppi_batch*, ccv_mppi_grid*, int32_t, int32_t*, int32_t*, double*);\n'
        'typedef int (*read_fn)(ccv_mppi_batch*, int32_t, float*);\n'
        'int main(void){static const float cells[6] = {1, 2, 3, 4, 5, 6};\n'
        'ccv_mppi_grid g = {0.0, 0.0, 0.05, -1.0f, 3, 2, cells};\n'
        'set_fn a = ccv_mppi_batch_set_grids; get_fn b = ccv_mppi_batch_get_grids; read_fn c = ccv_mppi_batch_read_grid_cells;\n'
        'return (a && b && c && g.nx * g.ny == 6 && CCV_MPPI_BATCH_KERNEL_GRID == 512 && CCV_MPPI_GRID_MAX_DIM == 32768) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_grid.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    cells = np.ones((2, 3), dtype=np.float32)
    g = (capi.Grid * 1)(capi.Grid(0.0, 0.0, 0.1, -1.0, 3, 2, cells.ctypes.data_as(C.POINTER(C.c_float))))
    mo, w, n = np.zeros(1, dtype=np.int32), np.ones(1), C.c_int32(0)
    ip = mo.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ccv_mppi_batch_set_grids(None, g, 1, ip, capi.dptr(w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_grids(None, None, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_grids(None, g, 1, C.byref(n), ip, capi.dptr(w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_grid_cells(None, 0, cells.ctypes.data_as(C.POINTER(C.c_float))) == capi.ERR_INVALID_ARG


def test_the_python_class_offers_the_term():
    assert callable(BatchController.set_grids) and callable(BatchController.get_grids)

"""CPU checks of the batch handles' device-inflated costmaps (ccv_mppi_batch_set_occupancy / _update_occupancy_enqueue /
_get_occupancy / _read_occupancy, struct ccv_mppi_occupancy, struct ccv_mppi_inflation): declared in the
public header, exported by the library, mirrored by the ctypes table and the Python class, the structs' layout against
capi.Occupancy and capi.Inflation through a compiled C program, the header still C99, a null handle refused, the new units in
the build.  (The refusals that need a handle: tests/test_gpu_batch_costmap.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
CALLS = {"ccv_mppi_batch_set_occupancy", "ccv_mppi_batch_update_occupancy_enqueue", "ccv_mppi_batch_get_occupancy",
         "ccv_mppi_batch_read_occupancy"}
OCC_FIELDS = ["origin_x", "origin_y", "resolution", "outside", "nx", "ny", "threshold", "cells"]
INF_FIELDS = ["radius", "free_value", "profile"]
u8p, i32p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)


def test_costmap_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert CALLS <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    assert not any("_resident_" in name for name in CALLS)
    lib = C.CDLL(build.build())
    for name in CALLS:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES and capi.SIGNATURES[name][0] is C.c_int
    assert capi.SIGNATURES["ccv_mppi_batch_set_occupancy"][1][1:] == [C.POINTER(capi.Occupancy), C.POINTER(capi.Inflation), C.c_int32, i32p,
                                                                       C.POINTER(C.c_double)]
    assert capi.SIGNATURES["ccv_mppi_batch_update_occupancy_enqueue"][1][1:] == [C.c_int32] * 5 + [u8p]
    assert capi.SIGNATURES["ccv_mppi_batch_get_occupancy"][1][1:] == [C.POINTER(capi.Occupancy), C.POINTER(capi.Inflation), C.c_int32, i32p]
    assert capi.SIGNATURES["ccv_mppi_batch_read_occupancy"][1][1:] == [C.c_int32, u8p]


def test_the_constants_are_the_headers():
    text = open(HEADER).read()
    assert capi.INFLATE_MAX_RADIUS == int(re.search(r"#define CCV_MPPI_INFLATE_MAX_RADIUS (\d+)", text).group(1)) == 64
    assert re.search(r"#define CCV_MPPI_OCC_PATCH_MAX_CELLS \(1 << 20\)", text) and capi.OCC_PATCH_MAX_CELLS == 1 << 20
    assert capi.OCC_PATCH_SLOTS == int(re.search(r"#define CCV_MPPI_OCC_PATCH_SLOTS (\d+)", text).group(1)) >= 2


def test_the_header_says_what_the_calls_promise():
    text = re.sub(r"\s*\n \* ", " ", open(HEADER).read())
    for phrase in ("cells[iy * nx + ix] >= threshold", "D2 <= R * R ? profile[D2] : free_value", "a cell outside the map is not occupied",
                   "no synchronisation, no allocation, no flush of a pending resident update",
                   "copied out of the caller's buffer before the call returns", "drops the occupancy layers",
                   "ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue below"):
        assert phrase in text, phrase


def test_the_struct_layouts_are_the_ctypes_mirrors(tmp_path):
    src = tmp_path / "occ_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ccv_mppi.h"\n'
                   'int main(void){printf("%zu", sizeof(ccv_mppi_occupancy));\n' +
                   "".join('printf(" %%zu", offsetof(ccv_mppi_occupancy, %s));\n' % f for f in OCC_FIELDS) +
                   'printf(" %zu", sizeof(ccv_mppi_inflation));\n' +
                   "".join('printf(" %%zu", offsetof(ccv_mppi_inflation, %s));\n' % f for f in INF_FIELDS) + 'return 0;}\n')
    exe = tmp_path / "occ_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert [f for f, _ in capi.Occupancy._fields_] == OCC_FIELDS and [f for f, _ in capi.Inflation._fields_] == INF_FIELDS
    assert got == ([C.sizeof(capi.Occupancy)] + [getattr(capi.Occupancy, f).offset for f in OCC_FIELDS] +
                   [C.sizeof(capi.Inflation)] + [getattr(capi.Inflation, f).offset for f in INF_FIELDS])


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_occ.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, const ccv_mppi_occupancy*, const ccv_mppi_inflation*, int32_t, const int32_t*, const double*);\n'
        'typedef int (*upd_fn)(ccv_mppi_batch*, int32_t, int32_t, int32_t, int32_t, int32_t, const uint8_t*);\n'
        'typedef int (*get_fn)(ccv_mppi_batch*, ccv_mppi_occupancy*, ccv_mppi_inflation*, int32_t, int32_t*);\n'
        'typedef int (*read_fn)(ccv_mppi_batch*, int32_t, uint8_t*);\n'
        'int main(void){static const uint8_t cells[6] = {0, 0, 255, 0, 0, 0}; static const float profile[2] = {1.0f, 0.5f};\n'
        'ccv_mppi_occupancy g = {0.0, 0.0, 0.05, -1.0f, 3, 2, 128, cells}; ccv_mppi_inflation f = {1, 0.0f, profile};\n'
        'set_fn a = ccv_mppi_batch_set_occupancy; upd_fn b = ccv_mppi_batch_update_occupancy_enqueue;\n'
        'get_fn c = ccv_mppi_batch_get_occupancy; read_fn d = ccv_mppi_batch_read_occupancy;\n'
        'return (a && b && c && d && g.nx * g.ny == 6 && f.radius == 1 && CCV_MPPI_INFLATE_MAX_RADIUS == 64 &&\n'
        '        CCV_MPPI_OCC_PATCH_MAX_CELLS == 1048576 && CCV_MPPI_OCC_PATCH_SLOTS >= 2) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_occ.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    cells, prof = np.ones((2, 3), dtype=np.uint8), np.ones(2, dtype=np.float32)
    g = (capi.Occupancy * 1)(capi.Occupancy(0.0, 0.0, 0.1, -1.0, 3, 2, 1, cells.ctypes.data_as(u8p)))
    f = (capi.Inflation * 1)(capi.Inflation(1, 0.0, prof.ctypes.data_as(f32p)))
    mo, w, n = np.zeros(1, dtype=np.int32), np.ones(1), C.c_int32(0)
    assert lib.ccv_mppi_batch_set_occupancy(None, g, f, 1, mo.ctypes.data_as(i32p), capi.dptr(w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_occupancy(None, None, None, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_update_occupancy_enqueue(None, 0, 0, 0, 3, 2, cells.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_occupancy(None, g, f, 1, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_occupancy(None, 0, cells.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_units():
    for name in ("set_occupancy", "update_occupancy", "get_occupancy", "read_occupancy"):
        assert callable(getattr(BatchController, name))
    assert callable(batch.inflation_profile)
    assert "k_costmap.hip" in build.KERNEL_UNITS and "mppi_costmap.h" in build.HEADERS
    assert "capi_batch_maps.hip" in build.CAPI_UNITS and "mppi_costmap_device.h" in build.HEADERS

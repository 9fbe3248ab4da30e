"""CPU checks of the batch handles' scan tracing (ccv_mppi_batch_scan_occupancy_enqueue): declared in the
public header, exported by the library, mirrored by the ctypes table and the Python class, the header still C99, a null handle
refused, the new unit in the build.  (The refusals that need a handle: tests/test_gpu_batch_scan.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
CALL = "ccv_mppi_batch_scan_occupancy_enqueue"
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def test_the_symbol_is_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert CALL in set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    proto = re.search(CALL + r"\s*\(([^;]*)\)\s*;", src).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "ccv_mppi_batch* b", "int32_t n", "const int32_t* map", "const int32_t* sensor_xy", "const int32_t* n_rays", "const int32_t* end_xy",
        "const uint8_t* hit", "int32_t clear_value", "int32_t mark_value"]
    assert hasattr(C.CDLL(build.build()), CALL), "libccv_mppi_hip.so does not export %s" % CALL
    assert capi.SIGNATURES[CALL][0] is C.c_int
    assert capi.SIGNATURES[CALL][1][1:] == [C.c_int32, i32p, i32p, i32p, i32p, u8p, C.c_int32, C.c_int32]
    assert re.search(r"#define\s+CCV_MPPI_SCAN_MAX_REACH\s+4096\b", src) and capi.SCAN_MAX_REACH == 4096


def test_the_header_says_what_the_call_promises():
    text = re.sub(r"\s*\n \* ", " ", open(HEADER).read())
    for phrase in ("the major axis is x if adx >= ady, else y", "minor = s_minor + sign_minor * ((2 * i * b + a) div (2 * a))",
                   "the end cell (i = a) is not part of the ray", "a ray with a = 0 has no cells", "(after ALL clears of that map)",
                   "marks win over clears within a call, whatever the order of the rays and of the entries", "skipped, never wrapped",
                   "what a fresh _set_occupancy of `new` would produce", "clipped to the map, grown by R and clipped again",
                   "no synchronisation, no allocation, no flush of a pending resident update", "two kernel launches however many maps it scans",
                   "a call in which nothing is traced launches nothing", "9 bytes per ray", "128 bytes per entry that has rays",
                   "the largest call of one entry has 116 494 rays", "Nothing changes either way"):
        assert phrase in text, phrase
    # the figures of the header are the layout's
    assert (capi.SCAN_RAY_BYTES, capi.SCAN_ENTRY_BYTES) == (9, 128)
    assert (capi.OCC_PATCH_MAX_CELLS - capi.SCAN_ENTRY_BYTES) // capi.SCAN_RAY_BYTES == 116494
    assert 64 * (capi.SCAN_ENTRY_BYTES + 360 * capi.SCAN_RAY_BYTES) == 215552


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_scan.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*scan_fn)(ccv_mppi_batch*, int32_t, const int32_t*, const int32_t*, const int32_t*, const int32_t*, const uint8_t*,\n'
        '                       int32_t, int32_t);\n'
        'int main(void){static const int32_t map[2] = {0, 1}, sensor[2][2] = {{5, 5}, {1, 2}}, n_rays[2] = {2, 1};\n'
        'static const int32_t end_xy[3][2] = {{9, 5}, {5, -3}, {1, 2}}; static const uint8_t hit[3] = {1, 0, 1};\n'
        'scan_fn f = ccv_mppi_batch_scan_occupancy_enqueue;\n'
        'return (f && CCV_MPPI_SCAN_MAX_REACH == 4096 && f(NULL, 2, map, &sensor[0][0], n_rays, &end_xy[0][0], hit, 0, 255) == CCV_MPPI_ERR_INVALID_ARG) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_scan.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    m, s, k = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int32), np.ones(1, dtype=np.int32)
    e, h = np.ones(2, dtype=np.int32), np.ones(1, dtype=np.uint8)
    assert lib.ccv_mppi_batch_scan_occupancy_enqueue(None, 1, m.ctypes.data_as(i32p), s.ctypes.data_as(i32p), k.ctypes.data_as(i32p),
                                                     e.ctypes.data_as(i32p), h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_scan_occupancy_enqueue(None, 0, None, None, None, None, None, 0, 255) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_call_and_the_build_has_the_unit():
    assert callable(BatchController.scan_occupancy) and callable(batch.scan_cells)
    assert "k_costmap_scan.hip" in build.KERNEL_UNITS and "mppi_costmap_scan.h" in build.HEADERS
    assert "k_costmap_roll.hip" in build.KERNEL_UNITS and "k_costmap.hip" in build.KERNEL_UNITS
    for name in ("k_costmap_scan.hip", "mppi_costmap_scan.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name

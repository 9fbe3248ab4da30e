"""CPU checks of the batch handles' simulated range sensor (ccv_mppi_batch_set_world, _resident_sense_enqueue and their four
companions): declared in the public header, exported by the library, mirrored by the ctypes table and the
Python class, the header still C99, a null handle refused, the new unit in the build.  (The refusals that need a handle:
tests/test_gpu_batch_sense.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
SENSE_HEADER = os.path.join(ROOT, "include", "ccv_mppi_sense.h")
u8p, i32p, occp = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(capi.Occupancy)
CALLS = {
    "ccv_mppi_batch_set_world": (["ccv_mppi_batch* b", "const ccv_mppi_occupancy* world", "const int32_t* anchor_xy", "int32_t max_beams"],
                                 [occp, i32p, C.c_int32]),
    "ccv_mppi_batch_get_world": (["ccv_mppi_batch* b", "ccv_mppi_occupancy* world", "int32_t* anchor_xy", "int32_t max_maps", "int32_t* max_beams"],
                                 [occp, i32p, C.c_int32, i32p]),
    "ccv_mppi_batch_read_world": (["ccv_mppi_batch* b", "uint8_t* out"], [u8p]),
    "ccv_mppi_batch_update_world_enqueue": (["ccv_mppi_batch* b", "int32_t x0", "int32_t y0", "int32_t w", "int32_t h", "const uint8_t* patch"],
                                            [C.c_int32, C.c_int32, C.c_int32, C.c_int32, u8p]),
    "ccv_mppi_batch_resident_sense_enqueue": (["ccv_mppi_batch* b", "int32_t n", "const int32_t* instance", "int32_t n_beams", "const int32_t* beam_xy",
                                               "int32_t clear_value", "int32_t mark_value"], [C.c_int32, i32p, C.c_int32, i32p, C.c_int32, C.c_int32]),
    "ccv_mppi_batch_resident_read_sense": (["ccv_mppi_batch* b", "int32_t* first", "int32_t* sensor_cell"], [i32p, i32p]),
}


def test_the_symbols_are_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read() + open(SENSE_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    # the two resident calls stand in ccv_mppi_sense.h, which ccv_mppi.h includes, and in a ctypes table of their own
    sense = re.sub(r"/\*.*?\*/", "", open(SENSE_HEADER).read(), flags=re.S)
    assert set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", sense)) == set(capi.SENSE_SIGNATURES) == {c for c in CALLS if "_resident_" in c}
    assert not set(capi.SENSE_SIGNATURES) & set(capi.SIGNATURES) and '#include "ccv_mppi_sense.h"' in open(HEADER).read()
    tables = dict(capi.SIGNATURES, **capi.SENSE_SIGNATURES)
    for call, (params, ctypes_args) in CALLS.items():
        assert call in declared, call
        proto = re.search(call + r"\s*\(([^;]*)\)\s*;", src).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == params, call
        assert hasattr(lib, call), "libccv_mppi_hip.so does not export %s" % call
        assert tables[call][0] is C.c_int and tables[call][1][1:] == ctypes_args, call
    assert re.search(r"#define\s+CCV_MPPI_SENSE_MAX_BEAMS\s+4096\b", src) and capi.SENSE_MAX_BEAMS == 4096


def test_the_header_says_what_the_calls_promise():
    text = re.sub(r"\s*\n \* ", " ", open(HEADER).read())
    for phrase in ("a cell outside the world is not occupied", "is never a cost term", "must have the world's resolution bit for bit",
                   "the world cell (ax + cx, ay + cy) at call time", "no floating point enters the frame change",
                   "the pose the last enqueued tick rolled out from", "(one subtraction, one multiplication, no FMA)",
                   "senses nothing: no cell of its map changes and its rectangle is empty", "(the sensor's own cell is not tested)",
                   "cell a being the end cell", "(after ALL clears of that map)", "a prefix of the beam's own line, not the line re-traced to cell f",
                   "skipped, never wrapped; the sensor's local cell may lie outside its map", "what a fresh _set_occupancy of the new layer would produce",
                   "clipped to the map, grown by R and clipped again", "the box holds the sensor cell and every end cell",
                   "no synchronisation, no allocation, no flush of a pending resident update", "two kernel launches however many robots sense",
                   "8 bytes per beam and 112 bytes per entry", "two named instances on one map", "a later call's marks win over an earlier call's clears",
                   "Nothing changes either way", "Only the rows of instances named by a call are written", "an anchor beyond +-2^29",
                   "(the anchors speak of those layers)", "the ground truth can change under a running fleet"):
        assert phrase in text, phrase
    # the figures of the header are the layout's: the largest call of B entries still has room for every beam
    assert (capi.SENSE_BEAM_BYTES, capi.SENSE_ENTRY_BYTES) == (8, 112)
    assert capi.SENSE_MAX_BEAMS * capi.SENSE_BEAM_BYTES + 8192 * capi.SENSE_ENTRY_BYTES <= capi.OCC_PATCH_MAX_CELLS


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_sense.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*sense_fn)(ccv_mppi_batch*, int32_t, const int32_t*, int32_t, const int32_t*, int32_t, int32_t);\n'
        'int main(void){static const int32_t inst[2] = {0, 1}, beams[3][2] = {{9, 5}, {5, -3}, {0, 0}}, anchor[2][2] = {{0, 0}, {3, 4}};\n'
        'static const uint8_t cells[6] = {0, 1, 0, 0, 0, 1}; ccv_mppi_occupancy w = {0.0, 0.0, 0.05, 0.0f, 3, 2, 1, cells};\n'
        'ccv_mppi_occupancy got; int32_t first[2 * 3], cell[2][2], mb; uint8_t out[6];\n'
        'sense_fn f = ccv_mppi_batch_resident_sense_enqueue;\n'
        'int bad = CCV_MPPI_SENSE_MAX_BEAMS != 4096;\n'
        'bad |= ccv_mppi_batch_set_world(NULL, &w, &anchor[0][0], 3) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_get_world(NULL, &got, NULL, 0, &mb) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_read_world(NULL, out) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_update_world_enqueue(NULL, 0, 0, 3, 2, cells) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= f(NULL, 2, inst, 3, &beams[0][0], 0, 255) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_read_sense(NULL, first, &cell[0][0]) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'return bad;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_sense.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    cells = np.zeros(6, dtype=np.uint8)
    w = capi.Occupancy(0.0, 0.0, 0.05, 0.0, 3, 2, 1, cells.ctypes.data_as(u8p))
    a, inst, beams = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32), np.ones(2, dtype=np.int32)
    assert lib.ccv_mppi_batch_set_world(None, C.byref(w), a.ctypes.data_as(i32p), 8) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_world(None, None, None, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_world(None, None, None, 0, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_world(None, cells.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_update_world_enqueue(None, 0, 0, 3, 2, cells.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_sense_enqueue(None, 1, inst.ctypes.data_as(i32p), 1, beams.ctypes.data_as(i32p), 0, 255) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_sense_enqueue(None, 0, None, 0, None, 0, 255) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_sense(None, None, None) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_unit():
    for name in ("set_world", "get_world", "read_world", "update_world", "resident_sense", "resident_read_sense"):
        assert callable(getattr(BatchController, name)), name
    assert callable(batch.beam_fan)
    assert "k_costmap_sense.hip" in build.KERNEL_UNITS and "mppi_costmap_sense.h" in build.HEADERS
    assert any(h.endswith("ccv_mppi_sense.h") for h in build.HEADERS)
    assert not any(u.startswith("k_batch") for u in build.KERNEL_UNITS if "sense" in u)
    assert "capi_batch_maps.hip" in build.CAPI_UNITS
    for name in ("k_costmap_sense.hip", "mppi_costmap_sense.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name

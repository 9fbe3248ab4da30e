"""CPU checks of the batch handles' rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue): declared in
the public header, exported by the library, mirrored by the ctypes table and the Python class, the header still C99, a null
handle refused, the new unit in the build, and the strip packing of the Python side against tests/roll_reference.py.  (The
refusals that need a handle: tests/test_gpu_batch_roll.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import roll_reference as RR
from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
CALL = "ccv_mppi_batch_roll_occupancy_enqueue"
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def test_the_symbol_is_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert CALL in set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    assert hasattr(C.CDLL(build.build()), CALL), "libccv_mppi_hip.so does not export %s" % CALL
    assert capi.SIGNATURES[CALL][0] is C.c_int
    assert capi.SIGNATURES[CALL][1][1:] == [C.c_int32, i32p, i32p, i32p, u8p, C.c_int32]


def test_the_header_says_what_the_call_promises():
    text = re.sub(r"\s*\n \* ", " ", open(HEADER).read())
    for phrase in ("new(ix, iy) = old(ix + dx, iy + dy)", "origin_x = origin0_x + (double)cx * resolution", "never by repeated addition",
                   "what a fresh _set_occupancy of `new` at the new origin would produce",
                   "first the row strip and then the column strip", "A 5 x 4 map (nx = 5, ny = 4) rolled by (dx, dy) = (2, -1)",
                   "no synchronisation, no flush of a pending resident update", "two kernel launches however many maps it rolls",
                   "336 * m bytes plus the strips", "the priming call, which changes no bit", "Nothing changes either way"):
        assert phrase in text, phrase


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_roll.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*roll_fn)(ccv_mppi_batch*, int32_t, const int32_t*, const int32_t*, const int32_t*, const uint8_t*, int32_t);\n'
        'int main(void){static const int32_t map[2] = {0, 1}, dx[2] = {2, 0}, dy[2] = {-1, 0};\n'
        'static const uint8_t exposed[11] = {0}; roll_fn f = ccv_mppi_batch_roll_occupancy_enqueue;\n'
        'return (f && f(NULL, 2, map, dx, dy, exposed, 0) == CCV_MPPI_ERR_INVALID_ARG) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_roll.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    m, d = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32)
    assert lib.ccv_mppi_batch_roll_occupancy_enqueue(None, 1, m.ctypes.data_as(i32p), d.ctypes.data_as(i32p), d.ctypes.data_as(i32p), None, 0) \
        == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_roll_occupancy_enqueue(None, 0, None, None, None, None, 0) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_call_and_the_build_has_the_unit():
    assert callable(BatchController.roll_occupancy) and callable(batch.pack_exposed)
    assert "k_costmap_roll.hip" in build.KERNEL_UNITS and "mppi_costmap_roll.h" in build.HEADERS
    assert "k_costmap.hip" in build.KERNEL_UNITS and "mppi_costmap.h" in build.HEADERS


def test_the_python_packing_is_the_references():
    sizes = [(5, 4), (5, 4), (3, 3), (7, 2), (1, 1), (4, 6)]
    moves = [(2, -1), (-2, 1), (0, 0), (-9, 1), (1, 0), (0, 7)]
    wins = [np.random.default_rng(i).integers(0, 256, size=(ny, nx)).astype(np.uint8) for i, (nx, ny) in enumerate(sizes)]
    entries = [RR.strips_of(w, dx, dy) for w, (dx, dy) in zip(wins, moves)]
    dx, dy = [m[0] for m in moves], [m[1] for m in moves]
    got = batch.pack_exposed(sizes, dx, dy, entries)
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, RR.pack_strips(entries))
    assert np.array_equal(batch.pack_exposed(sizes[:1], dx[:1], dy[:1], entries[:1]), [*wins[0][0], *wins[0][1:, 3:].reshape(-1)])
    # an empty strip may be None; a strip of another shape is refused
    assert np.array_equal(batch.pack_exposed([(5, 4)], [2], [0], [(None, wins[0][:, 3:])]), wins[0][:, 3:].reshape(-1))
    with pytest.raises(ValueError):
        batch.pack_exposed(sizes[:1], dx[:1], dy[:1], [(entries[0][0], entries[0][1][:2])])
    with pytest.raises(ValueError):
        batch.pack_exposed(sizes[:2], dx[:2], dy[:2], entries[:1])

"""CPU checks of the costmaps that follow their robots (ccv_mppi_batch_resident_set_follow, _follow_enqueue and their three
companions): declared in a public header of their own, exported by the library, mirrored by a ctypes table
of their own and the Python class, the header still C99, a null handle refused, the new units in the build.  (The refusals that
need a handle: tests/test_gpu_batch_follow.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
FOLLOW_HEADER = os.path.join(ROOT, "include", "ccv_mppi_follow.h")
i32p, i64p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
CALLS = {
    "ccv_mppi_batch_resident_set_follow": (["ccv_mppi_batch* b", "int32_t on"], [C.c_int32]),
    "ccv_mppi_batch_resident_get_follow": (["ccv_mppi_batch* b", "int32_t* on"], [i32p]),
    "ccv_mppi_batch_resident_follow_enqueue": (["ccv_mppi_batch* b", "int32_t n", "const int32_t* instance", "int32_t margin", "int32_t max_step",
                                                "int32_t fill"], [C.c_int32, i32p, C.c_int32, C.c_int32, C.c_int32]),
    "ccv_mppi_batch_resident_read_follow": (["ccv_mppi_batch* b", "int32_t* status", "int32_t* shift", "int64_t* offset", "double* origin"],
                                            [i32p, i32p, i64p, dp]),
    "ccv_mppi_batch_resident_plan_goals_enqueue": (["ccv_mppi_batch* b", "int32_t n", "const int32_t* instance", "const double* goal_xy", "float lethal",
                                                    "int32_t max_sweeps"], [C.c_int32, i32p, dp, C.c_float, C.c_int32]),
}
STATUS = {"MOVED": 1, "HELD": 2, "NO_POSE": 3, "LIMIT": 4}


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_the_symbols_are_declared_exported_and_in_a_ctypes_table_of_their_own():
    follow = _code(FOLLOW_HEADER)
    lib = C.CDLL(build.build())
    assert set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", follow)) == set(capi.FOLLOW_SIGNATURES) == set(CALLS)
    # the prototypes do not stand in ccv_mppi.h, which includes the header after the planner's
    main = open(HEADER).read()
    assert not set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", _code(HEADER))) & set(CALLS)
    assert main.index('#include "ccv_mppi_plan.h"') < main.index('#include "ccv_mppi_follow.h"')
    others = set(capi.SIGNATURES) | set(capi.FLEET_SIGNATURES) | set(capi.SENSE_SIGNATURES) | set(capi.PLAN_SIGNATURES)
    assert not set(capi.FOLLOW_SIGNATURES) & others
    for call, (params, ctypes_args) in CALLS.items():
        proto = re.search(call + r"\s*\(([^;]*)\)\s*;", follow).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == params, call
        assert hasattr(lib, call), "libccv_mppi_hip.so does not export %s" % call
        assert capi.FOLLOW_SIGNATURES[call][0] is C.c_int and capi.FOLLOW_SIGNATURES[call][1][1:] == ctypes_args, call
    for name, value in STATUS.items():
        assert re.search(r"#define\s+CCV_MPPI_FOLLOW_%s\s+%d\b" % (name, value), follow) and getattr(capi, "FOLLOW_" + name) == value, name


def test_the_headers_say_what_the_calls_promise():
    text = re.sub(r"\s*\n \* +", " ", open(HEADER).read())
    for phrase in ("Costmaps that follow their robots (NOT reference behaviour; off until called; batch handles and resident steps only)",
                   "decided on the device: the host reads no pose", "one subtraction, one multiplication, no FMA", "false for a NaN or infinite pose",
                   "floor, not truncation", "C integer division: the centre cell", "each axis on its own", "nothing moves",
                   "one multiplication, one addition, no FMA: the host roll's formula", "0: the map has never been followed",
                   "equal in every bit what ccv_mppi_batch_roll_occupancy_enqueue(m, dx, dy, exposed = NULL, fill) leaves",
                   "On every other status no bit of the layer, the float cells, the origin or any tick changes",
                   "a named map changes to its second set of buffers", "the device's frame is the truth", "_roll_occupancy_enqueue returns CCV_MPPI_ERR_STATE",
                   "synchronise and show the device's frame", "_set_occupancy, _set_grids and destroy drop following",
                   "Needs occupancy (CCV_MPPI_ERR_STATE otherwise)", "host rolls work again and no bit of any tick changes",
                   "two kernel launches however many: no synchronisation, no allocation, no flush of a pending resident update, no copy",
                   "two named instances on one map", "margin outside [0, CCV_MPPI_GRID_MAX_DIM]", "max_step outside [1, CCV_MPPI_GRID_MAX_DIM]",
                   "fill outside [0, 255]", "Following not set, or no resident poses: CCV_MPPI_ERR_STATE", "Nothing changes either way",
                   "any pointer may be NULL", "f < 0 -> 0, f >= n -> n - 1, else (int)f", "a goal that is not finite: CCV_MPPI_ERR_INVALID_ARG",
                   "Everything else is _plan_enqueue's"):
        assert phrase in text, phrase
    own = open(FOLLOW_HEADER).read()
    assert "clamp(e, -max_step, max_step)" in own and '#include "ccv_mppi.h"' in own


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_follow.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*follow_fn)(ccv_mppi_batch*, int32_t, const int32_t*, int32_t, int32_t, int32_t);\n'
        'int main(void){static const int32_t inst[1] = {0}; static const double goal[1][2] = {{1.0, 2.0}};\n'
        'int32_t on, status[2], shift[2][2]; int64_t offset[2][2]; double origin[2][2];\n'
        'follow_fn f = ccv_mppi_batch_resident_follow_enqueue;\n'
        'int bad = CCV_MPPI_FOLLOW_MOVED != 1 || CCV_MPPI_FOLLOW_HELD != 2 || CCV_MPPI_FOLLOW_NO_POSE != 3 || CCV_MPPI_FOLLOW_LIMIT != 4;\n'
        'bad |= ccv_mppi_batch_resident_set_follow(NULL, 1) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_get_follow(NULL, &on) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= f(NULL, 1, inst, 2, 3, 0) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_read_follow(NULL, status, &shift[0][0], &offset[0][0], &origin[0][0]) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_plan_goals_enqueue(NULL, 1, inst, &goal[0][0], 0.5f, 100) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'return bad;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_follow.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    a, d, n = np.zeros(4, dtype=np.int32), np.zeros(4), C.c_int32(0)
    o = np.zeros(4, dtype=np.int64)
    ip = a.ctypes.data_as(i32p)
    assert lib.ccv_mppi_batch_resident_set_follow(None, 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_set_follow(None, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_get_follow(None, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_follow_enqueue(None, 1, ip, 1, 1, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_follow(None, ip, ip, o.ctypes.data_as(i64p), capi.dptr(d)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_plan_goals_enqueue(None, 1, ip, capi.dptr(d), 0.5, 10) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_units():
    for name in ("resident_set_follow", "resident_get_follow", "resident_follow", "resident_read_follow", "resident_plan_goals"):
        assert callable(getattr(BatchController, name)), name
    shift = batch.follow_shift(((-3.0, 1.5), 0.25, 9, 6), [[-1.875, 2.375], [-1.125, 1.6], [9.0, -9.0], [np.nan, 2.0]], 2, 5)
    assert shift.dtype == np.int32 and shift.tolist() == [[0, 0], [3, -3], [5, -5], [0, 0]]
    assert "k_costmap_follow.hip" in build.KERNEL_UNITS and "capi_batch_follow.hip" in build.CAPI_UNITS
    assert "mppi_costmap_follow.h" in build.HEADERS and "mppi_costmap_follow_decide.h" in build.HEADERS
    assert any(h.endswith("ccv_mppi_follow.h") for h in build.HEADERS)
    for name in ("k_costmap_follow.hip", "mppi_costmap_follow.h", "mppi_costmap_follow_decide.h", "capi_batch_follow.hip"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    # following is a part of the handle that owns its memory by type
    internal = open(os.path.join(build.CSRC, "capi_internal.h")).read()
    assert "struct Follow {" in internal and "DeviceArray<FollowFrame> d_follow_frames" in internal
    assert re.search(r"struct ccv_mppi_batch : [^{]*\bFollow\b", internal)
    # the kernels the sensor and the planner already had are not touched: the followed forms are launches of their own
    for unit in ("k_costmap_sense.hip", "k_plan.hip"):
        assert "mppi_costmap_follow" not in open(os.path.join(build.CSRC, unit)).read(), unit

"""CPU checks of the batch handles' device planner (ccv_mppi_batch_resident_set_plan, _plan_enqueue and their four companions;
DESIGN.md section 10q): declared in a public header of their own, exported by the library, mirrored by a ctypes table of their
own and the Python class, the header still C99, a null handle refused, the new units in the build.  (The refusals that need a
handle: tests/test_gpu_batch_plan.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
PLAN_HEADER = os.path.join(ROOT, "include", "ccv_mppi_plan.h")
i32p, u16p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_double)
CALLS = {
    "ccv_mppi_batch_resident_set_plan": (["ccv_mppi_batch* b", "const int32_t* capacity", "int32_t keep_fields"], [i32p, C.c_int32]),
    "ccv_mppi_batch_resident_get_plan": (["ccv_mppi_batch* b", "int32_t* capacity", "int32_t* keep_fields"], [i32p, i32p]),
    "ccv_mppi_batch_resident_plan_enqueue": (["ccv_mppi_batch* b", "int32_t n", "const int32_t* instance", "const int32_t* goal_xy", "float lethal",
                                              "int32_t max_sweeps"], [C.c_int32, i32p, i32p, C.c_float, C.c_int32]),
    "ccv_mppi_batch_resident_read_plan": (["ccv_mppi_batch* b", "int32_t* status", "int32_t* poses", "int32_t* start_cell", "int32_t* start_dist",
                                           "int32_t* sweeps"], [i32p] * 5),
    "ccv_mppi_batch_resident_read_plan_field": (["ccv_mppi_batch* b", "int32_t instance", "uint16_t* out"], [C.c_int32, u16p]),
    "ccv_mppi_batch_resident_read_path": (["ccv_mppi_batch* b", "int32_t instance", "int32_t max_poses", "double* x", "double* y", "int32_t* n_path"],
                                          [C.c_int32, C.c_int32, dp, dp, i32p]),
}
STATUS = {"OK": 1, "TRUNCATED": 2, "NO_START": 3, "START_BLOCKED": 4, "GOAL_BLOCKED": 5, "UNREACHABLE": 6, "NOT_CONVERGED": 7}


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_the_symbols_are_declared_exported_and_in_a_ctypes_table_of_their_own():
    plan = _code(PLAN_HEADER)
    lib = C.CDLL(build.build())
    assert set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", plan)) == set(capi.PLAN_SIGNATURES) == set(CALLS)
    # the prototypes do not stand in ccv_mppi.h, which includes the header after the sensor's
    main = open(HEADER).read()
    assert not set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", _code(HEADER))) & set(CALLS)
    assert main.index('#include "ccv_mppi_sense.h"') < main.index('#include "ccv_mppi_plan.h"')
    assert not set(capi.PLAN_SIGNATURES) & (set(capi.SIGNATURES) | set(capi.FLEET_SIGNATURES) | set(capi.SENSE_SIGNATURES))
    for call, (params, ctypes_args) in CALLS.items():
        proto = re.search(call + r"\s*\(([^;]*)\)\s*;", plan).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == params, call
        assert hasattr(lib, call), "libccv_mppi_hip.so does not export %s" % call
        assert capi.PLAN_SIGNATURES[call][0] is C.c_int and capi.PLAN_SIGNATURES[call][1][1:] == ctypes_args, call
    assert re.search(r"#define\s+CCV_MPPI_PLAN_MAX_FIELD\s+81920\b", plan) and capi.PLAN_MAX_FIELD == 81920
    assert re.search(r"#define\s+CCV_MPPI_PLAN_MAX_POSES\s+16384\b", plan) and capi.PLAN_MAX_POSES == 16384
    for name, value in STATUS.items():
        assert re.search(r"#define\s+CCV_MPPI_PLAN_%s\s+%d\b" % (name, value), plan) and getattr(capi, "PLAN_" + name) == value, name


def test_the_headers_say_what_the_calls_promise():
    text = re.sub(r"\s*\n \* +", " ", open(HEADER).read())
    for phrase in ("Paths planned on the device (NOT reference behaviour; off until called; batch handles and resident steps only)",
                   "a NaN cell is blocked, a cell equal to lethal is free", "outside the map is blocked", "a straight move has weight 5, a diagonal move weight 7",
                   "no corner cutting; the rule is symmetric", "65533 means both \"not reached\" and \"farther than 65532\"",
                   "whatever order the device relaxes in", "one subtraction, one multiplication, no FMA", "the host reads no pose",
                   "in the order E, N, W, S, NE, NW, SW, SE", "start and goal included", "one multiplication, one addition, no FMA",
                   "pose 0 is the start cell", "sqrt(2) * resolution apart", "on every other status no bit of the path, n_path or the next tick changes",
                   "converges whenever max_sweeps >= J", "nx * ny + 1 is always enough", "below J the outcome is the device's own",
                   "(nx + 2)(ny + 2) <= CCV_MPPI_PLAN_MAX_FIELD", "must equal its map's resolution bit for bit", "no bit of any tick changes",
                   "capacity == NULL turns planning off", "so does a later _resident_set_paths", "_resident_set_poses keeps every instance's path",
                   "two may share a map, which is only read", "one kernel launch: no synchronisation, no allocation, no flush of a pending resident update, no copy",
                   "Nothing changes either way", "while the instance's last status is not 1, 2 or 6", "planned or set"):
        assert phrase in text, phrase
    own = open(PLAN_HEADER).read()
    assert "sqrt(2) * resolution apart" in own and '#include "ccv_mppi.h"' in own


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_plan.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*plan_fn)(ccv_mppi_batch*, int32_t, const int32_t*, const int32_t*, float, int32_t);\n'
        'int main(void){static const int32_t cap[2] = {64, 0}, inst[1] = {0}, goal[1][2] = {{3, 4}};\n'
        'int32_t got[2], keep, status[2], poses[2], cell[2][2], dist[2], sweeps[2], n; uint16_t field[6]; double x[4], y[4];\n'
        'plan_fn f = ccv_mppi_batch_resident_plan_enqueue;\n'
        'int bad = CCV_MPPI_PLAN_MAX_FIELD != 81920 || CCV_MPPI_PLAN_MAX_POSES != 16384 || CCV_MPPI_PLAN_OK != 1 || CCV_MPPI_PLAN_NOT_CONVERGED != 7;\n'
        'bad |= ccv_mppi_batch_resident_set_plan(NULL, cap, 1) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_get_plan(NULL, got, &keep) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= f(NULL, 1, inst, &goal[0][0], 0.5f, 100) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_read_plan(NULL, status, poses, &cell[0][0], dist, sweeps) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_read_plan_field(NULL, 0, field) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_read_path(NULL, 0, 4, x, y, &n) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'return bad;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_plan.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    a, d, n = np.zeros(4, dtype=np.int32), np.zeros(4), C.c_int32(0)
    f = np.zeros(4, dtype=np.uint16)
    ip = a.ctypes.data_as(i32p)
    assert lib.ccv_mppi_batch_resident_set_plan(None, ip, 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_set_plan(None, None, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_get_plan(None, ip, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_plan_enqueue(None, 1, ip, ip, 0.5, 10) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_plan(None, ip, ip, ip, ip, ip) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_plan_field(None, 0, f.ctypes.data_as(u16p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_path(None, 0, 4, capi.dptr(d), capi.dptr(d), C.byref(n)) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_units():
    for name in ("resident_set_plan", "resident_get_plan", "resident_plan", "resident_read_plan", "resident_read_plan_field", "resident_read_path"):
        assert callable(getattr(BatchController, name)), name
    cells = batch.goal_cells(((-3.0, 1.5), 0.25, 7, 5), [[-3.0, 1.5], [-2.74, 2.6], [9.0, -9.0], [np.nan, 2.0]])
    assert cells.dtype == np.int32 and cells.tolist() == [[0, 0], [1, 4], [6, 0], [0, 2]]
    assert "k_plan.hip" in build.KERNEL_UNITS and "capi_batch_plan.hip" in build.CAPI_UNITS and "mppi_plan.h" in build.HEADERS
    assert any(h.endswith("ccv_mppi_plan.h") for h in build.HEADERS)
    for name in ("k_plan.hip", "mppi_plan.h", "capi_batch_plan.hip"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    # the staging ring is declared where every enqueueing unit sees it, and defined once
    # (StagingRing, csrc/capi_owned.h, which capi_internal.h includes; the handle's part Staging holds the one the calls share)
    internal, owned = (open(os.path.join(build.CSRC, name)).read() for name in ("capi_internal.h", "capi_owned.h"))
    assert '#include "capi_owned.h"' in internal and "struct Staging" in internal and "hipError_t staging_create(" in internal
    for name in ("struct Slot", "class StagingRing", "hipError_t create(", "hipError_t take(", "hipError_t seal("):
        assert name in owned, name
    sources = [f for f in sorted(os.listdir(build.CSRC)) if f.endswith((".h", ".hip"))]
    defined = [f for f in sources if re.search(r"^\s*hipError_t take\(Slot& .*\{$", open(os.path.join(build.CSRC, f)).read(), re.M)]
    assert defined == ["capi_owned.h"]

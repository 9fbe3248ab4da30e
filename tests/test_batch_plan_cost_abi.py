"""CPU checks of the traversal weights of the device planner (ccv_mppi_batch_resident_set_plan_penalty, _get_plan_penalty;
DESIGN.md section 10t): declared in a public header of their own, exported by the library, mirrored by a ctypes table of their
own and the Python class, the header still C99, a null handle refused, the new units in the build.  (The refusals that need a
handle: tests/test_gpu_batch_plan_cost.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
COST_HEADER = os.path.join(ROOT, "include", "ccv_mppi_plan_cost.h")
i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
CALLS = {
    "ccv_mppi_batch_resident_set_plan_penalty": (["ccv_mppi_batch* b", "float gain", "int32_t max_penalty"], [C.c_float, C.c_int32]),
    "ccv_mppi_batch_resident_get_plan_penalty": (["ccv_mppi_batch* b", "float* gain", "int32_t* max_penalty"], [fp, i32p]),
}


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_the_symbols_are_declared_exported_and_in_a_ctypes_table_of_their_own():
    cost = _code(COST_HEADER)
    lib = C.CDLL(build.build())
    assert set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", cost)) == set(capi.PLAN_COST_SIGNATURES) == set(CALLS)
    # the prototypes stand in no other header; ccv_mppi.h includes the new one after the follower's
    main = open(HEADER).read()
    for other in ("ccv_mppi.h", "ccv_mppi_plan.h", "ccv_mppi_follow.h", "ccv_mppi_sense.h", "ccv_mppi_fleet.h", "ccv_mppi_host.h"):
        assert not set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", _code(os.path.join(ROOT, "include", other)))) & set(CALLS), other
    assert main.index('#include "ccv_mppi_follow.h"') < main.index('#include "ccv_mppi_plan_cost.h"')
    others = set(capi.SIGNATURES) | set(capi.FLEET_SIGNATURES) | set(capi.SENSE_SIGNATURES) | set(capi.PLAN_SIGNATURES) | set(capi.FOLLOW_SIGNATURES)
    assert not set(capi.PLAN_COST_SIGNATURES) & others
    for call, (params, ctypes_args) in CALLS.items():
        proto = re.search(call + r"\s*\(([^;]*)\)\s*;", cost).group(1)
        assert [" ".join(a.split()) for a in proto.split(",")] == params, call
        assert hasattr(lib, call), "libccv_mppi_hip.so does not export %s" % call
        assert capi.PLAN_COST_SIGNATURES[call][0] is C.c_int and capi.PLAN_COST_SIGNATURES[call][1][1:] == ctypes_args, call
    assert re.search(r"#define\s+CCV_MPPI_PLAN_MAX_PENALTY\s+15\b", cost) and capi.PLAN_MAX_PENALTY == 15


def test_the_headers_say_what_the_calls_promise():
    text = re.sub(r"\s*\n \* +", " ", open(HEADER).read())
    for phrase in ("Paths planned on the device: traversal weights (NOT reference behaviour; off until called; batch handles and resident steps only)",
                   "t = cell(c) * gain", "one fp32 multiplication, round to nearest, no FMA",
                   "q(c) = !(t > 0) ? 0 : (t >= (float)max_penalty ? max_penalty : (int)t)", "a NaN t gives 0", "m(c) = 1 + q(c)",
                   "step(c -> n) = w(c, n) * m(c)", "the cell that is left is charged, not the cell entered", "the move rule is no longer symmetric",
                   "every cell on it but the goal charged, the start included", "D(n) + step(c -> n) == D(c)",
                   "the sweeps of the weighted Jacobi iteration", "D still falls by at least 5 a step",
                   "With max_penalty == 0 or gain == 0 every multiplier is 1", "from the same kernel as before",
                   "a NaN, infinite or negative gain or a max_penalty outside the range: CCV_MPPI_ERR_INVALID_ARG, and nothing changes",
                   "Needs _resident_set_plan (CCV_MPPI_ERR_STATE otherwise)", "Host state only: no synchronisation, no allocation, no launch",
                   "every later _plan_enqueue and _plan_goals_enqueue", "A fresh _set_plan starts at (0, 0)",
                   "_set_plan(NULL), _resident_set_paths, destroy", "report the weighted plan", "either pointer may be NULL"):
        assert phrase in text, phrase
    own = open(COST_HEADER).read()
    assert "(t >= (float)max_penalty ? max_penalty : (int)t)" in own and '#include "ccv_mppi.h"' in own


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_plan_cost.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, float, int32_t);\n'
        'int main(void){float gain; int32_t max_penalty;\n'
        'set_fn f = ccv_mppi_batch_resident_set_plan_penalty;\n'
        'int bad = CCV_MPPI_PLAN_MAX_PENALTY != 15;\n'
        'bad |= f(NULL, 8.0f, CCV_MPPI_PLAN_MAX_PENALTY) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'bad |= ccv_mppi_batch_resident_get_plan_penalty(NULL, &gain, &max_penalty) != CCV_MPPI_ERR_INVALID_ARG;\n'
        'return bad;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_plan_cost.o")], check=True)
    # ... and with the new header alone
    alone = tmp_path / "alone.c"
    alone.write_text('#include "ccv_mppi_plan_cost.h"\nint main(void){return ccv_mppi_batch_resident_set_plan_penalty(0, 1.0f, 1) == CCV_MPPI_OK;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(alone),
                    "-o", str(tmp_path / "alone.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    g, m = C.c_float(0.0), C.c_int32(0)
    assert lib.ccv_mppi_batch_resident_set_plan_penalty(None, 8.0, 15) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_set_plan_penalty(None, 0.0, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_get_plan_penalty(None, C.byref(g), C.byref(m)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_get_plan_penalty(None, None, None) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_units():
    for name in ("resident_set_plan_penalty", "resident_get_plan_penalty"):
        assert callable(getattr(BatchController, name)), name
    m = batch.plan_multiplier(np.array([[0.0, 0.124, 0.125, 0.5], [-1.0, np.nan, 0.74, np.inf]], dtype=np.float32), 8.0, 4)
    assert m.dtype == np.int32 and m.tolist() == [[1, 1, 2, 5], [1, 1, 5, 5]]
    assert "k_plan_cost.hip" in build.KERNEL_UNITS and "mppi_plan_cost.h" in build.HEADERS and "mppi_plan_penalty.h" in build.HEADERS
    assert any(h.endswith("ccv_mppi_plan_cost.h") for h in build.HEADERS)
    for name in ("k_plan_cost.hip", "mppi_plan_cost.h", "mppi_plan_penalty.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    # the quantisation is a header without HIP in it: the stand-alone host program compiles the device's own lines
    penalty = open(os.path.join(build.CSRC, "mppi_plan_penalty.h")).read()
    assert "hip_runtime" not in penalty and "__host__ __device__" in penalty
    assert '#include "mppi_plan_penalty.h"' in open(os.path.join(ROOT, "tools", "plan_penalty_check.cpp")).read()
    # the unweighted kernel's unit knows nothing of the weights; the weighted kernel is a unit of its own, chosen by the host
    plain = open(os.path.join(build.CSRC, "k_plan.hip")).read()
    assert "plan_cost" not in plain and "plan_penalty" not in plain and "k_plan_field_cost" not in plain
    host = open(os.path.join(build.CSRC, "capi_batch_plan.hip")).read()
    assert host.count("launch_plan_field_cost(") == 1 and host.count("launch_plan_field(") == 1 and host.count("launch_plan(bh, ") == 2
    # the setting belongs to the handle's part Plan
    internal = open(os.path.join(build.CSRC, "capi_internal.h")).read()
    part = internal[internal.index("struct Plan {"):internal.index("void drop_plan()")]
    assert "plan_gain" in part and "plan_max_penalty" in part

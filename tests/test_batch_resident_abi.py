"""CPU checks of the batch handles' device-resident closed loop (ccv_mppi_batch_resident_*): declared in the public header,
exported by the library, mirrored by the ctypes table, and a null handle refused by every entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ccv_mppi_path_tracker_amd import BatchController, build, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
RESIDENT = {"ccv_mppi_batch_resident_set_paths", "ccv_mppi_batch_resident_set_poses", "ccv_mppi_batch_resident_step_enqueue",
            "ccv_mppi_batch_resident_read", "ccv_mppi_batch_resident_read_trace"}


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(ccv_mppi_batch_resident_[a-z_0-9]+)\s*\(", src))


def test_resident_batch_symbols_are_declared_exported_and_in_the_ctypes_table():
    declared = _declared()
    assert declared == RESIDENT
    lib = C.CDLL(build.build())
    for name in RESIDENT:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
    assert RESIDENT == {n for n in capi.SIGNATURES if n.startswith("ccv_mppi_batch_resident_")}


def test_resident_batch_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_resident.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_paths_fn)(ccv_mppi_batch*, const double*, const double*, const int32_t*, const double*);\n'
        'typedef int (*set_poses_fn)(ccv_mppi_batch*, const double*, const uint64_t*);\n'
        'typedef int (*step_fn)(ccv_mppi_batch*, double, uint64_t, int32_t);\n'
        'typedef int (*read_fn)(ccv_mppi_batch*, double*, int32_t*, double*, double*, double*, int64_t*);\n'
        'typedef int (*trace_fn)(ccv_mppi_batch*, int32_t, int32_t, double*, int32_t*);\n'
        'int main(void){set_paths_fn a = ccv_mppi_batch_resident_set_paths; set_poses_fn b = ccv_mppi_batch_resident_set_poses;\n'
        'step_fn c = ccv_mppi_batch_resident_step_enqueue; read_fn d = ccv_mppi_batch_resident_read;\n'
        'trace_fn e = ccv_mppi_batch_resident_read_trace;\n'
        'return (a && b && c && d && e && CCV_MPPI_BATCH_TRACE_ROWS >= 1) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_resident.o")], check=True)
    assert capi.BATCH_TRACE_ROWS == int(re.search(r"#define CCV_MPPI_BATCH_TRACE_ROWS (\d+)", open(HEADER).read()).group(1))


def test_a_null_batch_handle_is_refused_by_every_resident_entry_point():
    lib = capi.load()
    d = (C.c_double * 64)()
    n = (C.c_int32 * 4)(1, 1, 1, 1)
    s = (C.c_uint64 * 4)()
    i32, i64 = C.c_int32(), C.c_int64()
    assert lib.ccv_mppi_batch_resident_set_paths(None, d, d, n, d) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_set_poses(None, d, s) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_step_enqueue(None, 0.1, 0, 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read(None, d, n, d, d, d, C.byref(i64)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read(None, None, None, None, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_trace(None, 0, 4, d, C.byref(i32)) == capi.ERR_INVALID_ARG


def test_resident_batch_has_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    with pytest.raises(MPPIError) as ei:
        BatchController(configs.diff_drive_defaults(64, 15), 4)
    assert ei.value.code == capi.ERR_NO_DEVICE
    assert hasattr(BatchController, "resident_step_enqueue") and hasattr(BatchController, "resident_read_trace")


def test_resident_batch_python_checks_shapes_before_the_library():
    """The shape checks run before the handle is used: a controller object without a handle shows them."""
    bc = BatchController.__new__(BatchController)
    bc.B, bc.H, bc.nstate = 3, 15, 3
    bc.params = configs.diff_drive_defaults(64, 15)
    with pytest.raises(ValueError):
        bc.resident_set_paths([(np.zeros(4), np.zeros(4))] * 2)          # 2 paths for 3 instances
    with pytest.raises(ValueError):
        bc.resident_set_paths([(np.zeros(4), np.zeros(5))] * 3)          # x and y of different lengths
    with pytest.raises(ValueError):
        bc.resident_set_paths([(np.zeros(0), np.zeros(0))] * 3)          # empty
    with pytest.raises(ValueError):
        bc.resident_set_poses(np.zeros((2, 3)), 1)                      # 2 poses for 3 instances
    with pytest.raises(ValueError):
        bc.resident_set_poses(np.zeros((3, 6)), 1)                      # 6 state entries

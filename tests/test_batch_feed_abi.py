"""CPU checks of the batch handles' feed calls (ccv_mppi_batch_read_best_candidates / _read_optimal_paths; DESIGN.md section
10l): declared in the public header, exported by the library, mirrored by the ctypes table and the Python class, the limit
against capi.BEST_MAX, the header's promises, the header still C99, a null handle refused, the new units in the build, the select
probe cross-compiled.  (The refusals that need a handle: tests/test_gpu_batch_feed.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import select_probe
from ccv_mppi_path_tracker_amd import BatchController, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
CALLS = {"ccv_mppi_batch_read_best_candidates", "ccv_mppi_batch_read_optimal_paths"}
i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def test_feed_symbols_are_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert CALLS <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in CALLS:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES and capi.SIGNATURES[name][0] is C.c_int
    assert capi.SIGNATURES["ccv_mppi_batch_read_best_candidates"][1][1:] == [C.c_int32, i32p, f64p, f64p]
    assert capi.SIGNATURES["ccv_mppi_batch_read_optimal_paths"][1][1:] == [f64p]


def test_the_limit_is_the_headers():
    text = open(HEADER).read()
    assert capi.BEST_MAX == int(re.search(r"#define CCV_MPPI_BEST_MAX (\d+)", text).group(1)) == 1024
    select_h = open(os.path.join(build.CSRC, "mppi_select.h")).read()
    assert int(re.search(r"constexpr int kSelectMax = (\d+);", select_h).group(1)) == 1024


def test_the_header_says_what_the_calls_promise():
    text = re.sub(r"\s*\n \* ", " ", open(HEADER).read())
    for phrase in ("Selection is by cost, not by weight", "Costs ascend, ties go to the lower sample index, NaN costs come last",
                   "every NaN 0xFFFFFFFFFFFFFFFF, -0.0 as +0.0, otherwise bits ^ (sign ? ~0 : 1 << 63)",
                   "lexsort((arange(K), cost))", "it does not flush a pending resident update",
                   "a resident tick keeps its two launches", "Only samples 0..K-1 take part",
                   "flushes a pending resident update as ccv_mppi_batch_get_nominal does",
                   "row i = the state BEFORE control step i", "count == 0 is OK and writes nothing",
                   "sorts nothing on the host and copies nothing to the device"):
        assert phrase in text, phrase


def test_a_c99_caller_compiles(tmp_path):
    src = tmp_path / "batch_feed.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*best_fn)(ccv_mppi_batch*, int32_t, int32_t*, double*, double*);\n'
        'typedef int (*path_fn)(ccv_mppi_batch*, double*);\n'
        'int main(void){int32_t idx[CCV_MPPI_BEST_MAX]; best_fn a = ccv_mppi_batch_read_best_candidates;\n'
        'path_fn b = ccv_mppi_batch_read_optimal_paths; idx[0] = 0;\n'
        'return (a && b && idx[0] == 0 && CCV_MPPI_BEST_MAX == 1024) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_feed.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    idx, cost, xy = np.zeros(4, dtype=np.int32), np.zeros(4), np.zeros((4, 15, 2))
    assert lib.ccv_mppi_batch_read_best_candidates(None, 4, idx.ctypes.data_as(i32p), capi.dptr(cost), capi.dptr(xy)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_best_candidates(None, 0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_optimal_paths(None, capi.dptr(xy)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_optimal_paths(None, None) == capi.ERR_INVALID_ARG


def test_the_python_side_offers_the_calls_and_the_build_has_the_units():
    for name in ("read_best_candidates", "read_optimal_paths"):
        assert callable(getattr(BatchController, name))
    assert "k_feed.hip" in build.KERNEL_UNITS and "capi_batch_feed.hip" in build.CAPI_UNITS
    assert "mppi_select.h" in build.HEADERS and "mppi_feed.h" in build.HEADERS


def test_the_select_probe_cross_compiles_and_sees_mppi_select_h_alone():
    text = open(select_probe.SOURCE).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["mppi_select.h"]
    assert not re.findall(r'#include\s+"([^"]+)"', open(os.path.join(build.CSRC, "mppi_select.h")).read())
    lib = C.CDLL(select_probe.build_probe())
    assert hasattr(lib, "probe_select")

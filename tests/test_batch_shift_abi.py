"""CPU checks of the batch handles' shifted-weight mode (ccv_mppi_batch_set_min_shift / _get_min_shift,
CCV_MPPI_BATCH_KERNEL_SHIFT): declared in the public header, exported by the library, mirrored by the ctypes table and the
Python class, a null handle refused, and the header still C99."""
import ctypes as C
import inspect
import os
import re
import subprocess

from ccv_mppi_path_tracker_amd import BatchController, build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
SHIFT = {"ccv_mppi_batch_set_min_shift", "ccv_mppi_batch_get_min_shift"}


def test_shift_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert SHIFT <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in SHIFT:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES
    assert capi.SIGNATURES["ccv_mppi_batch_set_min_shift"][1][1] is C.c_int32
    assert capi.BATCH_KERNEL_SHIFT == int(re.search(r"#define CCV_MPPI_BATCH_KERNEL_SHIFT (\d+)", text).group(1)) == 64
    # the SHIFT bit is distinct from the kernel codes, the wide-turn bit and the VARIED bit
    assert capi.BATCH_KERNEL_SHIFT & (capi.BATCH_KERNEL_ONE_WAVE | capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE |
                                      capi.BATCH_KERNEL_VARIED) == 0


def test_shift_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_shift.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, int32_t);\n'
        'typedef int (*get_fn)(const ccv_mppi_batch*);\n'
        'int main(void){set_fn a = ccv_mppi_batch_set_min_shift; get_fn b = ccv_mppi_batch_get_min_shift;\n'
        'return (a && b && CCV_MPPI_BATCH_KERNEL_SHIFT > CCV_MPPI_BATCH_KERNEL_VARIED) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_shift.o")], check=True)


def test_a_null_batch_handle_is_refused_by_set_and_get_min_shift():
    lib = capi.load()
    assert lib.ccv_mppi_batch_set_min_shift(None, 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_min_shift(None, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_min_shift(None) == capi.ERR_INVALID_ARG


def test_the_python_class_offers_the_mode():
    assert "min_shift" in inspect.signature(BatchController.__init__).parameters
    assert inspect.signature(BatchController.__init__).parameters["min_shift"].default is False
    assert callable(BatchController.set_min_shift) and callable(BatchController.get_min_shift)

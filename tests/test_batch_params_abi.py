"""CPU checks of the batch handles' per-instance parameters (ccv_mppi_batch_set_params / _get_params): declared in the public
header, exported by the library, mirrored by the ctypes table, a null handle refused, and the shared fields checked in Python
before the library is called."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ccv_mppi_path_tracker_amd import BatchController, build, capi, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
PARAMS = {"ccv_mppi_batch_set_params", "ccv_mppi_batch_get_params"}


def test_params_symbols_are_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert PARAMS <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in PARAMS:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES
    assert capi.BATCH_KERNEL_VARIED == int(re.search(r"#define CCV_MPPI_BATCH_KERNEL_VARIED (\d+)", open(HEADER).read()).group(1))
    # the VARIED bit is distinct from the kernel codes and the wide-turn bit
    assert capi.BATCH_KERNEL_VARIED & (capi.BATCH_KERNEL_ONE_WAVE | capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE) == 0


def test_params_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_params.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, const ccv_mppi_config*);\n'
        'typedef int (*get_fn)(ccv_mppi_batch*, ccv_mppi_config*);\n'
        'int main(void){set_fn a = ccv_mppi_batch_set_params; get_fn b = ccv_mppi_batch_get_params;\n'
        'return (a && b && CCV_MPPI_BATCH_KERNEL_VARIED > CCV_MPPI_BATCH_KERNEL_WIDE) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_params.o")], check=True)


def test_a_null_batch_handle_is_refused_by_set_and_get_params():
    lib = capi.load()
    cfgs = (capi.Config * 2)()
    assert lib.ccv_mppi_batch_set_params(None, cfgs) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_params(None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_params(None, cfgs) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_params(None, None) == capi.ERR_INVALID_ARG


class _NoLibrary:
    """Stands in for the library: any call fails the test (the Python checks must come first)."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("field,value", [("model", "steering_diff_drive"), ("horizon", 20), ("roll_off", True),
                                         ("steer_off", True), ("num_samples", 128)])
def test_disagreeing_shared_fields_raise_before_the_library(field, value):
    p = configs.diff_drive_defaults(64, 15)
    if field == "model":
        q = configs.steering_defaults(64, 15)
    else:
        q = p.with_(**{field: value})
    bc = BatchController.__new__(BatchController)
    bc.lib, bc._h = _NoLibrary(), capi._H()
    bc.B, bc.K, bc.H, bc.params, bc.params_list = 3, 64, 15, p, [p] * 3
    bc.device, bc.no_state_store = 0, False
    with pytest.raises(ValueError, match=field):
        bc.set_params([p, q, p])
    with pytest.raises(ValueError):
        bc.set_params([p, p])   # 2 parameter sets for 3 instances
    # ... and at construction, before a handle is created
    with pytest.raises(ValueError, match=field):
        BatchController([p, p.with_(lam=2.0), q], 3)


def test_per_instance_fields_may_differ():
    """The Python check passes sequences that differ only in per-instance fields (it then calls the library)."""
    from ccv_mppi_path_tracker_amd.batch import check_shared
    p = configs.full_body_defaults(64, 15)
    check_shared([p, p.with_(control_noise=0.1, lam=3.0, v_ref=0.4, u_min=(-1.0,) * 5, u_max=(2.0,) * 5, path_weight=2.0,
                             v_weight=0.5, zmp_weight=0.1, roll_v_weight=0.2, back_weight=4.0, yaw_weight=0.0,
                             dt=0.05, resolution=0.2)])

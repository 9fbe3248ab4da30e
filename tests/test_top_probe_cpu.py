"""CPU checks of the single handle's top-candidates selection as a unit: csrc/mppi_top_weights.h is in
the build, stands alone, holds the one key that the kernel and the host ordering both use; the public header says what the call
promises; the probe cross-compiles for gfx950 and sees that header alone; the host ordering, compiled for the CPU, is the
reference's.  (The device: tests/test_gpu_top_candidates.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import top_cases as Cs
import top_probe
import top_reference as R
from ccv_mppi_path_tracker_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = r'#include\s+"([^"]+)"'


def _csrc(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def test_the_header_is_in_the_build_and_stands_alone():
    assert "mppi_top_weights.h" in build.HEADERS
    text = _csrc("mppi_top_weights.h")
    assert not re.findall(INCLUDE, text)
    assert int(re.search(r"constexpr int kTopBlock = (\d+);", text).group(1)) == 1024
    assert "constexpr int kTopBlock" not in _csrc("mppi_update.h")   # (defined once, in the header the probe sees)


def test_kernel_and_host_order_by_the_one_key():
    header = re.sub(r"//.*", "", _csrc("mppi_top_weights.h"))
    assert len(re.findall(r"__host__ __device__ inline unsigned long long top_key\(", header)) == 1
    assert len(re.findall(r"\btop_key\(", header)) == 5          # its definition, two in the ordering, two in the kernel's passes
    for unit in ("k_update.hip", "capi_stage.hip"):
        text = re.sub(r"//.*", "", _csrc(unit))
        assert "mppi_top_weights.h" in re.findall(INCLUDE, text)
        assert "__double_as_longlong(w[" not in text and "reinterpret_cast<const long long*>" not in text and "std::sort" not in text
    assert "top_weights<kTopBlock>(" in _csrc("k_update.hip") and "top_order_pairs(" in _csrc("capi_stage.hip")


def test_the_public_header_says_what_the_call_promises():
    text = re.sub(r"\s*\n \* ", " ", open(os.path.join(ROOT, "include", "ccv_mppi.h")).read())
    assert "ties: lower sample index first; NaN weights first, by sample index among themselves" in text


def test_the_top_probe_cross_compiles_and_sees_mppi_top_weights_h_alone():
    assert re.findall(INCLUDE, open(top_probe.SOURCE).read()) == ["mppi_top_weights.h"]
    assert top_probe.DEPS == [top_probe.SOURCE, os.path.join(build.CSRC, "mppi_top_weights.h")]
    assert top_probe.command("x")[1:len(build.HIPCC_FLAGS) + 1] == build.HIPCC_FLAGS
    lib = C.CDLL(top_probe.build_probe())
    assert hasattr(lib, "probe_top")
    w = np.zeros(4)
    i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    a, b = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint64)
    args = (w.ctypes.data_as(C.POINTER(C.c_double)), a.ctypes.data_as(i32), b.ctypes.data_as(u64), a.ctypes.data_as(i32), b.ctypes.data_as(u64))
    for n_vec, pitch, k, n in ((0, 4, 4, 1), (1, 4, 5, 1), (1, 4, 4, 0), (1, 4, 4, 5), (1, 4, 0, 0)):   # (refused before any HIP call)
        assert lib.probe_top(n_vec, pitch, k, n, *args) == 1, (n_vec, pitch, k, n)


HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "mppi_top_weights.h"
// stdin: n, then n pairs (index, weight bits in hex); stdout: the pairs after top_order_pairs(), and top_key of every weight
int main() {
    int n;
    if (scanf("%d", &n) != 1) return 2;
    std::vector<int> idx(n);
    std::vector<double> w(n);
    for (int j = 0; j < n; ++j) {
        unsigned long long b;
        if (scanf("%d %llx", &idx[j], &b) != 2) return 2;
        memcpy(&w[j], &b, 8);
        printf("%llx\n", ccv::top_key(w[j]));
    }
    ccv::top_order_pairs(n, idx.data(), w.data());
    for (int j = 0; j < n; ++j) {
        unsigned long long b;
        memcpy(&b, &w[j], 8);
        printf("%d %llx\n", idx[j], b);
    }
    return 0;
}
"""


def test_the_host_ordering_compiled_for_the_cpu_is_the_references(tmp_path):
    """top_key() and top_order_pairs() as the host compiler builds them (hipcc, host side only, the product's flags), fed the kernel
    layout of the NaN mix, the two-valued and the subnormal inputs at K = 257: keys, order and weight bits are the reference's"""
    src, exe = tmp_path / "host_order.hip", tmp_path / "host_order"
    src.write_text(HOST_MAIN)
    flags = [f for f in build.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([build.hipcc()] + flags + ["-I", build.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True)
    checked = 0
    for name, N, vecs in Cs.all_inputs(257):
        if name not in ("nan_mix", "two_values_random", "subnormal", "all_equal") or N not in (2, 65, 257):
            continue
        for w in vecs:
            idx, wbits = R.kernel_layout(w, N)
            perm = np.random.default_rng(N).permutation(N)       # (the function must not rely on the layout's order)
            text = "%d\n" % N + "".join("%d %x\n" % (idx[j], wbits[j]) for j in perm)
            out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
            keys = np.array([int(x, 16) for x in out[:N]], dtype=np.uint64)
            np.testing.assert_array_equal(keys, R.key(w)[idx[perm]])
            got = [line.split() for line in out[N:2 * N]]
            want_idx, want_bits = R.top(w, N)
            np.testing.assert_array_equal(np.array([int(g[0]) for g in got]), want_idx, err_msg="%s N=%d" % (name, N))
            np.testing.assert_array_equal(np.array([int(g[1], 16) for g in got], dtype=np.uint64), want_bits)
            checked += 1
    assert checked == 36

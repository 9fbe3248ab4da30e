"""CPU test: the register budget of the four-wave rollout kernel's two flagship instantiations, from the compiler's own metadata.

k_r4.hip is compiled for the device only, to assembly, with the flags the library is built with (build.HIPCC_FLAGS); the test reads
two fields of each kernel's metadata record -- `.private_segment_fixed_size` (bytes of scratch per lane) and `.vgpr_spill_count` --
and nothing else of the file.

The budget: k_rollout_r4<diff drive, fused> (workload C2) and k_rollout_r4<steering, fused> (C3) park no vector register and use no
scratch.  With the compare-and-select clamp form inside the dynamics wave's loop they parked 41 and 21 registers (168 and 88 B);
with that form deleted outright -- the floor a compiler reaches when the form is absent, not a shippable kernel -- 4 and 0 (20 and
0 B).  Both forms are still there (mppi_rollout_r4.h: a loop per form, chosen once), and every other fused instantiation of the two
models in this unit (wide turns, the masked tail, the batch form) is held to the same budget.
"""
import os
import re
import subprocess

import pytest

from ccv_mppi_path_tracker_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# <MODEL, MODE, WIDE, TAIL, FORM, SHIFT> as the mangled names spell them
C2 = "k_rollout_r4ILi0ELi0ELb0ELb0ELNS_9BatchFormE0ELb0EEE"
C3 = "k_rollout_r4ILi1ELi0ELb0ELb0ELNS_9BatchFormE0ELb0EEE"
FLOOR = {C2: (4, 20), C3: (0, 0)}   # (spilled VGPRs, scratch bytes) with the compare-and-select form deleted


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "k_r4.s")
    flags = [f for f in build.HIPCC_FLAGS if f != "-fPIC"]
    subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", build.CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(build.CSRC, "k_r4.hip"), "-o", out], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = (field("vgpr_spill_count"), field("private_segment_fixed_size"))
    return meta


def find(meta, part):
    names = [n for n in meta if part in n]
    assert len(names) == 1, (part, names)
    return meta[names[0]]


@pytest.mark.parametrize("kernel", [C2, C3], ids=["C2_diff_drive", "C3_steering"])
def test_flagship_kernels_use_no_scratch(kernel_meta, kernel):
    spilled, scratch = find(kernel_meta, kernel)
    print(kernel, "spilled VGPRs", spilled, "scratch bytes", scratch)
    assert spilled <= FLOOR[kernel][0] and scratch <= FLOOR[kernel][1]   # (the issue's bound)
    assert (spilled, scratch) == (0, 0)                                 # (what the change reached)


def test_every_fused_two_wheel_instantiation_uses_no_scratch(kernel_meta):
    fused = {n: v for n, v in kernel_meta.items() if re.search(r"k_rollout_r4ILi[01]ELi0E", n)}
    assert len(fused) == 12, sorted(fused)   # (2 x 4 diff drive: wide x tail x single / batch; 2 x 2 steering)
    for name, (spilled, scratch) in sorted(fused.items()):
        print(name, "spilled VGPRs", spilled, "scratch bytes", scratch)
    assert all(v == (0, 0) for v in fused.values()), fused

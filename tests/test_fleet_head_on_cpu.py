"""CPU check of the parameters of the fleet term's head-on test (tests/test_gpu_batch_fleet.py, the behaviour test; DESIGN.md
section 10f): on the CPU restatement of the closed loop (tools/fleet_head_on_cpu.py) the two robots pass closer than the sum
of their radii with the term off and strictly farther apart with it on, with room to spare.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import fleet_head_on_cpu as HO  # noqa: E402
import fleet_support as FS  # noqa: E402


def test_the_head_on_parameters_separate_on_from_off_on_the_cpu_restatement():
    c = FS.HEAD_ON
    p = FS.params()
    off = HO.closest_approach(p, c["paths"], c["s0"], c["seeds"], c["ticks"], [c["radius"]] * 2, c["range"], None)
    on = HO.closest_approach(p, c["paths"], c["s0"], c["seeds"], c["ticks"], [c["radius"]] * 2, c["range"], c["weight"])
    print("closest approach off / on (CPU restatement): %.4f / %.4f" % (off, on))
    assert off < 2 * c["radius"] - 0.2   # the robots drive through one another, well inside the two radii
    assert on > off + 0.2                # and the term moves them apart by far more than the two arithmetics differ

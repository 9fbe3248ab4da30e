"""CPU check of the parameters of the fleet prediction's crossing test (tests/test_gpu_batch_moving.py, the behaviour test;
DESIGN.md section 10g): on the CPU restatement of the closed loop (tools/fleet_crossing_cpu.py) two robots on perpendicular
paths, timed to reach the crossing together, pass inside the two radii with the term off and with snapshot discs, and farther
apart with predicted discs -- by more than twice the margin the GPU test asserts.  No GPU.

The restatement's figures at these parameters (K = 128, shifted weights, radii 0.1 m + 0.1 m, range 3 m, weight 100, seeds 11 /
12, 60 ticks): off 0.0609 m, snapshot 0.0752 m, predicted 0.2407 m (range 1.5 m: 0.0752 / 0.2409; weight 50: 0.0694 / 0.2301,
weight 200: 0.0905 / 0.2470).  The margin, 0.08 m, is below half the gap of 0.1655 m."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import fleet_crossing_cpu as FC  # noqa: E402
import fleet_support as FS  # noqa: E402


def test_the_crossing_parameters_separate_predicted_from_snapshot_on_the_cpu_restatement():
    c = FS.CROSSING
    p = FS.params()
    res = {m: FC.closest_approach(p, c["paths"], c["s0"], c["seeds"], c["ticks"], [c["radius"]] * 2, c["range"], c["weight"], m)
           for m in ("off", "snapshot", "predicted")}
    print("closest approach off / snapshot / predicted (CPU restatement): %.4f / %.4f / %.4f" % (res["off"], res["snapshot"], res["predicted"]))
    assert res["off"] < 2 * c["radius"] and res["snapshot"] < 2 * c["radius"]   # both drive through the two radii
    assert res["predicted"] > res["snapshot"] + c["margin"]
    assert c["margin"] <= 0.5 * (res["predicted"] - res["snapshot"])             # the margin: at most half the gap shown here

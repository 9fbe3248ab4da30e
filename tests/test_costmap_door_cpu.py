"""CPU check of the parameters of the door test (tests/test_gpu_batch_costmap.py::test_a_door_closes): on
the CPU restatement of the closed loop (tools/costmap_door_cpu.py) the robot drives through the cells of the block while it is
never patched in, and keeps clear of them by more than a cell, going round, when it is patched in ahead of the horizon's
reach -- at every weight over a 50-fold range.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import costmap_door_cpu as CD  # noqa: E402
import costmap_reference as CR  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402


def test_the_scenario_is_what_it_says():
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    x0, y0, patch = CD.block_patch()
    assert patch.all() and patch.size <= 1 << 20 and x0 + patch.shape[1] <= CD.NX and y0 + patch.shape[0] <= CD.NY
    lo_y, hi_y = CD.ORIGIN[1] + y0 * CD.RESOLUTION, CD.ORIGIN[1] + (y0 + patch.shape[0]) * CD.RESOLUTION
    assert lo_y < 0.0 < hi_y and hi_y > 1.0 and lo_y > -0.3                       # across the path, a way round on one side only
    assert CD.ORIGIN[0] + x0 * CD.RESOLUTION - CD.START[0] > CD.reach(p)          # out of the horizon's reach at the start
    assert max(CD.WEIGHTS) / min(CD.WEIGHTS) >= 50.0 and CD.WEIGHT in CD.WEIGHTS
    R, profile, free = CD.inflation()
    assert R == 6 and profile[0] == 1.0 and free == 0.0 and np.all(np.diff(profile) <= 0.0)
    # the bare block under the transform: lethal on the block, a ring around it, nothing beyond R
    cost = CR.cost_separable(CR.apply_patch(CD.empty_layer(), x0, y0, patch), CD.THRESHOLD, R, profile, free)
    block = np.zeros(cost.shape, dtype=bool)
    block[y0:y0 + patch.shape[0], x0:x0 + patch.shape[1]] = True
    assert np.all(cost[block] == 1.0) and np.all(cost[~block] < 1.0) and cost[y0 - 1, x0] == 0.5 and cost[y0 - R - 1, x0] == 0.0
    assert not CD.costmap(CD.empty_layer()).cells.any()


def test_without_the_patch_the_robot_drives_through_the_blocks_cells():
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    off = CD.drive(p, CD.WEIGHT, False)
    print("no patch: %d poses in the block's cells, end x %.2f" % (CD.in_block(off), off[-1, 0]))
    assert CD.in_block(off) >= 3


@pytest.mark.parametrize("weight", CD.WEIGHTS)
def test_with_the_patch_the_robot_passes_the_block_by_more_than_a_cell(weight):
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    on = CD.drive(p, weight, True)   # (asserts that the block appears out of the horizon's reach)
    print("weight %g: %d poses in the block's cells, closest %.3f m, end x %.2f" % (weight, CD.in_block(on), CD.clearance(on), on[-1, 0]))
    assert CD.in_block(on) == 0
    assert CD.clearance(on) >= CD.RESOLUTION      # by at least one cell
    assert on[-1, 0] > CD.BLOCK["x1"]             # ... and past it

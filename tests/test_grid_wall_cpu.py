"""CPU check of the parameters of the occupancy-grid term's wall test (tests/test_gpu_batch_grid.py, the behaviour test;
DESIGN.md section 10h): on the CPU restatement of the closed loop (tools/grid_wall_cpu.py) the robot drives through the block
of occupied cells with the term off and round it with the term on, with room to spare.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import grid_wall_cpu as GW  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402


def test_the_wall_map_is_what_it_says():
    g = GW.wall_map(**GW.WALL)
    w = GW.WALL
    assert set(np.unique(g.cells).tolist()) == {0.0, 0.5, 1.0} and float(g.outside) == 0.0
    ys, xs = np.nonzero(g.cells == 1.0)
    cx, cy = g.ox + (xs + 0.5) * g.resolution, g.oy + (ys + 0.5) * g.resolution
    assert w["x0"] <= cx.min() and cx.max() <= w["x1"] and w["y0"] <= cy.min() and cy.max() <= w["y1"]
    assert cy.min() < 0.0 < cy.max()                      # the block lies across the path y = 0
    assert cy.max() > 1.0 and cy.min() > -0.2             # ... and extends to one side only
    assert GW.occupied(g, np.array([[3.0, 0.0], [3.0, -0.5], [1.0, 0.0], [9.0, 9.0]])) == 1


def test_the_wall_parameters_separate_on_from_off_on_the_cpu_restatement():
    p = configs.diff_drive_defaults(GW.SAMPLES, 15)
    g = GW.wall_map(**GW.WALL)
    off, on = GW.drive(p, g, None), GW.drive(p, g, GW.WEIGHT)
    corner = float(np.min(np.hypot(on[:, 0] - GW.WALL["x0"], on[:, 1] - GW.WALL["y0"])))
    print("poses in occupied cells off / on (CPU restatement): %d / %d; on: closest to the block's corner %.3f m, largest |y| %.3f m, "
          "end x %.2f" % (GW.occupied(g, off), GW.occupied(g, on), corner, float(np.max(np.abs(on[:, 1]))), on[-1, 0]))
    assert GW.occupied(g, off) >= 3            # the robot drives through the block
    assert GW.occupied(g, on) == 0
    assert corner > 0.15                       # ... and round it by far more than the two arithmetics differ
    assert on[-1, 0] > GW.WALL["x1"]           # ... and past it

#!/usr/bin/env python3
"""CPU restatement of the resident closed loop over a device-inflated costmap that is patched while the loop runs, for choosing
the parameters of the door test (tests/test_gpu_batch_costmap.py::test_a_door_closes; the method of
tools/grid_wall_cpu.py, section 10h).  No GPU.

One diff-drive robot on the straight 6 m path of the wall test, starting further back.  The map is empty occupancy under
batch.inflation_profile's ring.  After tick PATCH_TICK -- the robot still more than the horizon's reach (|v|max dt (H - 1)) short of
it -- a bare block of occupied cells is patched across the path (the wall test's rectangle, no hand-painted ring: the inflation
comes from the transform, tests/costmap_reference.py).  Every tick: the oracle's window, Philox samples, rollouts and cost plus
weight * G of tests/grid_reference.py over the costmap of that moment, shifted weights, u* = sum w u, the plant on u*[0].
The arithmetic is the oracle's and numpy's, not the device's: the figures serve to pick block, ring and weights with a margin.
Prints one line per weight: trace poses in the block's cells and the closest approach to the block, without and with the patch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import costmap_reference as CR  # noqa: E402
import grid_reference as GR  # noqa: E402
import grid_wall_cpu as GW  # noqa: E402
import helpers  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, configs  # noqa: E402
from oracle import oracle_lib as O  # noqa: E402

# the test's choice (main() prints the sweep it was taken from)
SAMPLES, TICKS, SEED = GW.SAMPLES, 140, GW.SEED
START = (0.8, 0.0, 0.0)
PATCH_TICK = 2                       # the patch is enqueued right after this tick's step
BLOCK = dict(GW.WALL, y0=-0.15)      # metres; the cells whose centre lies in it (the wall test's, further across the path)
ORIGIN, RESOLUTION, NX, NY = (0.0, -2.0), 0.05, 120, 80
THRESHOLD = 128
RING = dict(radius_m=0.3, kind="linear", lethal=1.0, inscribed=0.5, inscribed_m=0.15, free_value=0.0)
WEIGHTS = (8.0, 40.0, 400.0)         # a 50-fold range
WEIGHT = 40.0                        # the GPU test's


def inflation():
    return batch.inflation_profile(resolution=RESOLUTION, **RING)


def block_patch():
    """(x0, y0, patch uint8 [h][w]): the cells whose centre lies in BLOCK, all occupied"""
    cx = ORIGIN[0] + (np.arange(NX) + 0.5) * RESOLUTION
    cy = ORIGIN[1] + (np.arange(NY) + 0.5) * RESOLUTION
    xs = np.nonzero((cx >= BLOCK["x0"]) & (cx <= BLOCK["x1"]))[0]
    ys = np.nonzero((cy >= BLOCK["y0"]) & (cy <= BLOCK["y1"]))[0]
    return int(xs[0]), int(ys[0]), np.full((len(ys), len(xs)), 255, dtype=np.uint8)


def empty_layer():
    return np.zeros((NY, NX), dtype=np.uint8)


def costmap(layer):
    R, profile, free = inflation()
    return GR.Grid(CR.cost_separable(layer, THRESHOLD, R, profile, free), ORIGIN, RESOLUTION, 0.0)


def in_block(trace):
    """how many poses [n][2] lie in cells the patch occupies"""
    x0, y0, patch = block_patch()
    g = GR.Grid(CR.apply_patch(empty_layer(), x0, y0, patch).astype(np.float32), ORIGIN, RESOLUTION, 0.0)
    v, _, _ = GR.lookup(g, trace[:, 0], trace[:, 1])
    return int(np.sum(v > 0.0))


def clearance(trace):
    """the closest any pose comes to the rectangle of the block's cells, metres"""
    x0, y0, patch = block_patch()
    lo_x, hi_x = ORIGIN[0] + x0 * RESOLUTION, ORIGIN[0] + (x0 + patch.shape[1]) * RESOLUTION
    lo_y, hi_y = ORIGIN[1] + y0 * RESOLUTION, ORIGIN[1] + (y0 + patch.shape[0]) * RESOLUTION
    dx = np.maximum(np.maximum(lo_x - trace[:, 0], trace[:, 0] - hi_x), 0.0)
    dy = np.maximum(np.maximum(lo_y - trace[:, 1], trace[:, 1] - hi_y), 0.0)
    return float(np.min(np.hypot(dx, dy)))


def reach(p):
    return max(abs(p.u_min[0]), abs(p.u_max[0])) * p.dt * (p.horizon - 1)


def drive(p, weight, patched, ticks=TICKS):
    """the closed loop over the empty map; patched: the block appears after tick PATCH_TICK -> the poses [ticks + 1][2]"""
    px, py = GW.path()
    o = helpers.oracle_for(p)
    s = np.array(START, dtype=np.float64)
    g = costmap(empty_layer())
    x0, y0, patch = block_patch()
    trace = [s[:2].copy()]
    for it in range(ticks):
        _, xr, yr, yaw = O.calc_ref_path(px, py, s[0], s[1], p.v_ref, p.dt, p.resolution, p.horizon)
        o.sampling(int(SEED), rng="philox", iteration=it)
        o.predict_States(s, p.dt)
        o.calc_Weights(xr, yr, yaw[0])
        P = np.stack([o.states("x"), o.states("y")], axis=-1)[:, :GR.n_covered(p.model, p.horizon)]
        c = GR.cost_on(o.costs(), weight, GR.grid_sum(g, P))
        w = np.exp(-(c - c.min()) / p.lam)
        w /= w.sum()
        u = np.einsum("k,ktd->td", w, o.get_controls())
        o.set_nominal(u)
        s[:3] = helpers.plant(p.model, s[:3], u[0], p.dt)
        trace.append(s[:2].copy())
        if patched and it == PATCH_TICK:
            assert BLOCK["x0"] - s[0] > reach(p), "the robot is within the horizon's reach of the block when it appears"
            g = costmap(CR.apply_patch(empty_layer(), x0, y0, patch))
    return np.array(trace)


def main():
    p = configs.diff_drive_defaults(SAMPLES, 15)
    for weight in WEIGHTS:
        for patched in (False, True):
            t = drive(p, weight, patched)
            print("weight %6.0f %s: %d poses in the block's cells, closest %.3f m, largest |y| %.3f, end x %.2f"
                  % (weight, "patched" if patched else "no patch", in_block(t), clearance(t), float(np.max(np.abs(t[:, 1]))), t[-1, 0]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""CPU restatement of the resident closed loop with the fleet term, for choosing the parameters of the head-on test
(tests/test_gpu_batch_fleet.py::test_two_robots_head_on_pass_at_a_larger_distance).  No GPU.

Two diff-drive robots on the same straight 6 m path in opposite directions.  Every tick, per robot: the window
(oracle calc_ref_path), the oracle's Philox samples and rollouts, the oracle's cost plus the disc penalty of
tests/obstacle_reference.py over the rollout's states for the other robot's disc -- its position at the START of the tick,
radius r0 + r1, if it is within range --, shifted weights exp(-(c - min c) / lambda), u* = sum w u, and the plant on u*[0].
The arithmetic is the oracle's and numpy's, not the device's, so the figures are near the device's, not equal to them; they
serve to pick path, radii, weight and range with a margin.  Prints one line per candidate: closest approach off / on."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import obstacle_reference as OR  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402
from oracle import oracle_lib as O  # noqa: E402


def closest_approach(p, paths, s0, seeds, ticks, radius, reach, weight):
    """weight = None: the term off"""
    B = len(s0)
    orc = [helpers.oracle_for(p) for _ in range(B)]
    s = np.array(s0, dtype=np.float64)
    best = np.inf
    for it in range(ticks):
        q = s[:, :2].copy()   # the snapshot: every position of this tick is the pose at its start
        u0 = []
        for y in range(B):
            _, xr, yr, yaw = O.calc_ref_path(paths[y][0], paths[y][1], s[y, 0], s[y, 1], p.v_ref, p.dt, p.resolution, p.horizon)
            o = orc[y]
            o.sampling(int(seeds[y]), rng="philox", iteration=it)
            o.predict_States(s[y], p.dt)
            o.calc_Weights(xr, yr, yaw[0])
            c = o.costs()
            discs = [(q[j, 0], q[j, 1], radius[y] + radius[j]) for j in range(B)
                     if j != y and (q[j, 0] - q[y, 0]) ** 2 + (q[j, 1] - q[y, 1]) ** 2 <= reach * reach]
            if weight is not None and discs:
                P = np.stack([o.states("x"), o.states("y")], axis=-1)
                c = c + OR.penalty(P, discs, weight).sum(axis=-1).astype(np.float64)
            w = np.exp(-(c - c.min()) / p.lam)
            w /= w.sum()
            u = np.einsum("k,ktd->td", w, o.get_controls())
            o.set_nominal(u)
            u0.append(u[0])
        for y in range(B):
            s[y, :3] = helpers.plant(p.model, s[y, :3], u0[y], p.dt)
        best = min(best, float(np.hypot(*(s[0, :2] - s[1, :2]))))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=90)
    ap.add_argument("--samples", type=int, default=128)
    args = ap.parse_args()
    p = configs.diff_drive_defaults(args.samples, 15)
    x = 0.1 * np.arange(61)
    paths = [(x, np.zeros(61)), (x[::-1].copy(), np.zeros(61))]
    s0 = np.array([[1.5, 0.0, 0.0], [4.5, 0.0, np.pi]])
    seeds = [11, 12]
    off = closest_approach(p, paths, s0, seeds, args.ticks, [0.3, 0.3], 3.0, None)
    print("term off: closest approach %.4f m" % off)
    for r in (0.2, 0.3):
        for reach in (1.0, 3.0):
            for weight in (10.0, 50.0, 200.0, 1000.0):
                on = closest_approach(p, paths, s0, seeds, args.ticks, [r, r], reach, weight)
                print("radius %.1f + %.1f  range %.1f  weight %6.0f: closest approach %.4f m (off %.4f)" % (r, r, reach, weight, on, off))


if __name__ == "__main__":
    main()

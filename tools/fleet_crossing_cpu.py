#!/usr/bin/env python3
"""CPU restatement of the resident closed loop with the fleet term and its prediction, for choosing the parameters of the
crossing test (tests/test_gpu_batch_moving.py::test_two_robots_crossing_pass_at_a_larger_distance_with_prediction; DESIGN.md
section 10g).  A sibling of tools/fleet_head_on_cpu.py, whose method it keeps.  No GPU.

Two diff-drive robots on perpendicular straight paths, each 1.5 m from the crossing, timed to reach it together.  Every tick,
per robot: the window (oracle calc_ref_path), the oracle's Philox samples and rollouts, the oracle's cost plus, for the other
robot if it is within range, the disc penalty over the rollout's states -- mode "snapshot": tests/obstacle_reference.py, the
disc at the other robot's position at the START of the tick; mode "predicted": tests/moving_obstacle_reference.py, that disc
moving at the velocity the other robot had over its last tick (tests/fleet_velocity_reference.py) --, shifted weights
exp(-(c - min c) / lambda), u* = sum w u, and the plant on u*[0].  The arithmetic is the oracle's and numpy's, not the device's,
so the figures are near the device's, not equal to them; they serve to pick radii, weight and range with a margin.  Prints one
line per candidate: closest approach off / snapshot / predicted."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import fleet_velocity_reference as FV  # noqa: E402
import moving_obstacle_reference as MR  # noqa: E402
import obstacle_reference as OR  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402
from oracle import oracle_lib as O  # noqa: E402

_S = 0.1 * np.arange(61)
PATHS = [(_S, np.zeros(61)), (np.full(61, 3.0), _S - 3.0)]             # along x through (3, 0); along y through (3, 0)
S0 = np.array([[1.5, 0.0, 0.0], [3.0, -1.5, np.pi / 2]])


def closest_approach(p, paths, s0, seeds, ticks, radius, reach, weight, mode):
    """mode: "off", "snapshot" or "predicted" """
    B = len(s0)
    orc = [helpers.oracle_for(p) for _ in range(B)]
    s = np.array(s0, dtype=np.float64)
    v = np.zeros((B, 2))
    best = np.inf
    ks = np.arange(p.horizon)
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
            near = [j for j in range(B) if j != y and (q[j, 0] - q[y, 0]) ** 2 + (q[j, 1] - q[y, 1]) ** 2 <= reach * reach]
            if mode != "off" and near:
                discs = [(q[j, 0], q[j, 1], radius[y] + radius[j]) for j in near]
                P = np.stack([o.states("x"), o.states("y")], axis=-1)
                if mode == "predicted":
                    pen = MR.penalty(P, ks, p.dt, discs, v[near], weight)
                else:
                    pen = OR.penalty(P, discs, weight)
                c = c + pen.sum(axis=-1).astype(np.float64)
            w = np.exp(-(c - c.min()) / p.lam)
            w /= w.sum()
            u = np.einsum("k,ktd->td", w, o.get_controls())
            o.set_nominal(u)
            u0.append(u[0])
        for y in range(B):
            s[y, :3] = helpers.plant(p.model, s[y, :3], u0[y], p.dt)
        v = FV.velocity(q, s[:, :2], p.dt, True)
        best = min(best, float(np.hypot(*(s[0, :2] - s[1, :2]))))
    return best


def main():
    """the sweep DESIGN.md section 10g quotes; the test's point is radius 0.1, range 3, weight 100, seeds 11 / 12"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.1, 0.15, 0.2, 0.3])
    ap.add_argument("--ranges", type=float, nargs="+", default=[1.5, 3.0])
    ap.add_argument("--weights", type=float, nargs="+", default=[10.0, 50.0, 100.0, 200.0, 1000.0])
    ap.add_argument("--seeds", type=int, nargs="+", default=[11, 12, 21, 22], help="pairs: robot 0's and robot 1's noise seed")
    args = ap.parse_args()
    p = configs.diff_drive_defaults(args.samples, 15)
    for seeds in zip(args.seeds[0::2], args.seeds[1::2]):
        off = closest_approach(p, PATHS, S0, seeds, args.ticks, [0.1, 0.1], 3.0, None, "off")
        print("seeds %d / %d  term off: closest approach %.4f m" % (seeds + (off,)), flush=True)
        for r in args.radii:
            for reach in args.ranges:
                for weight in args.weights:
                    snap = closest_approach(p, PATHS, S0, seeds, args.ticks, [r, r], reach, weight, "snapshot")
                    pred = closest_approach(p, PATHS, S0, seeds, args.ticks, [r, r], reach, weight, "predicted")
                    print("seeds %d / %d  radius %.2f + %.2f  range %.1f  weight %6.0f: closest approach snapshot %.4f m, predicted %.4f m" % (
                        seeds + (r, r, reach, weight, snap, pred)), flush=True)


if __name__ == "__main__":
    main()

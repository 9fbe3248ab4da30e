#!/usr/bin/env python3
"""The weighted device planner (ccv_mppi_batch_resident_set_plan_penalty) against the unweighted one
(section 10q) in the same run and on the same inputs: `python tools/batch_plan_cost_timing.py [--out FILE]` (default
profiles/batch_plan_cost_timing.json).  The method and the resident loop (its costmap form) are those of tools/bench_support.py.

One robot on one 200 x 200 device-inflated costmap with a graded (linear, R = 6) profile -- empty, 3 % random, serpentine:
`plan_us`, one plan call between two events, median of the rounds with their spread, with the sweeps it took, its status and the
mean clearance of its path, once with every multiplier 1 (k_plan_field) and once with gain 8 / lethal, max_penalty 15
(k_plan_field_cost); `ratio` is weighted over unweighted, `ratio_per_sweep` the same per sweep.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 costmap per robot (2 % of the layer occupied): `none`, no
planning; `plan` and `plan_cost`, all 64 robots plan after every tick, in one call, each to the far corner of its own map.
Device events around --ticks ticks, us per tick, and the wall time of the same loop.

Clearance: the distance in cells from a path's cell to the nearest occupied cell of the layer, searched up to 20 cells (a path
farther than that from everything counts 20; null on a layer without an occupied cell).  Nothing here asserts a time.  One JSON
document goes to stdout (and --out)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(bs.ROOT, "tests"))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402
import plan_reference as PR  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
LETHAL = 0.9          # (above the profile's first ring, 1 - 1 / 6: only the occupied cells themselves are blocked)
GAIN, MAX_PENALTY = 8.0 / LETHAL, 15
RULES = (("unweighted", 0.0, 0), ("weighted", GAIN, MAX_PENALTY))
TICK_MODES = ("none", "plan", "plan_cost")
R, N, CAPACITY = 6, 200, 1024
REACH = 20
i32p = C.POINTER(C.c_int32)


def raw_plan(h, inst, goals, max_sweeps):
    rc = h.lib.ccv_mppi_batch_resident_plan_enqueue(h._h, len(inst), inst.ctypes.data_as(i32p), goals.ctypes.data_as(i32p), LETHAL, max_sweeps)
    assert rc == capi.OK, rc


def clearance_map(layer):
    """float [ny][nx]: the distance in cells to the nearest occupied cell (>= 128) within REACH, REACH beyond; None without one"""
    occ = layer >= 128
    if not occ.any():
        return None
    ny, nx = occ.shape
    x = np.arange(nx, dtype=np.float64)[None, :]
    left = x - np.maximum.accumulate(np.where(occ, x, -1.0e9), axis=1)
    right = np.minimum.accumulate(np.where(occ, x, 1.0e9)[:, ::-1], axis=1)[:, ::-1] - x
    row = np.minimum(np.minimum(left, right), float(REACH))
    best = np.full((ny, nx), float(REACH * REACH))
    for dy in range(-REACH, REACH + 1):
        lo, hi = max(0, -dy), min(ny, ny - dy)
        best[lo:hi] = np.minimum(best[lo:hi], row[lo + dy:hi + dy] ** 2 + float(dy * dy))
    return np.sqrt(np.minimum(best, float(REACH * REACH)))


def mean_clearance(clear, path, origin, res):
    if clear is None or len(path[0]) == 0:
        return None
    ix = np.clip(np.floor((path[0] - origin[0]) / res).astype(np.int64), 0, clear.shape[1] - 1)
    iy = np.clip(np.floor((path[1] - origin[1]) / res).astype(np.int64), 0, clear.shape[0] - 1)
    return float(clear[iy, ix].mean())


def one_plan(rounds):
    n, res = N, RESOLUTION
    p = configs.diff_drive_defaults(128, 15)
    kinds = {"empty": PR.empty(n, n), "random_0.03": np.where(np.random.default_rng(3).random((n, n)) < 0.03, 1.0, 0.0).astype(np.float32),
             "serpentine": PR.serpentine(n, n)}
    infl = bs.inflation(R, res)
    out = {"nx": n, "ny": n, "lethal": LETHAL, "R": R, "gain": GAIN, "max_penalty": MAX_PENALTY}
    for name, cells in kinds.items():
        cells[0, 0] = 0.0
        goal = PR.free_cell(cells[::-1, ::-1], 0.5, (0, 0))
        goals = np.array([[n - 1 - goal[0], n - 1 - goal[1]]], dtype=np.int32)
        if name == "serpentine":   # (half way up: the whole corridor is longer than the field can count)
            goals = np.array([[n // 2, n // 2]], dtype=np.int32)
        layer = np.where(cells > 0.5, 255, 0).astype(np.uint8)
        clear = clearance_map(layer)
        h = amd.BatchController(p, 1)
        stream = bs.new_stream()
        h.set_stream(stream.cuda_stream)
        h.resident_set_paths(amd.make_path("dkan"), res)
        h.resident_set_poses(np.array([[0.5 * res, 0.5 * res, 0.0]]), 1)
        h.set_occupancy([(layer, (0.0, 0.0), res, 0.0, 128)], infl, [0], W_GRID)
        h.resident_set_plan(capi.PLAN_MAX_POSES, False)
        inst = np.zeros(1, dtype=np.int32)
        row = {"goal": goals[0].tolist()}
        for rule, gain, max_penalty in RULES:
            h.resident_set_plan_penalty(gain, max_penalty)
            raw_plan(h, inst, goals, n * n + 1)   # (warm-up)
            h.synchronize()
            ms, us = bs.one_call_ms_and_us(h, stream, rounds, lambda: raw_plan(h, inst, goals, n * n + 1))
            us["spread"] = float(max(us["rounds"]) - min(us["rounds"]))
            status, poses, _cell, dist, sweeps = h.resident_read_plan()
            row[rule] = {"status": int(status[0]), "poses": int(poses[0]), "start_dist": int(dist[0]), "sweeps": int(sweeps[0]), "plan_ms": ms, "plan_us": us,
                         "us_per_sweep": us["median"] / max(int(sweeps[0]), 1),
                         "mean_clearance_cells": mean_clearance(clear, h.resident_read_path(0), (0.0, 0.0), res) if status[0] in (1, 2) else None}
        h.close()
        row["ratio"] = row["weighted"]["plan_us"]["median"] / row["unweighted"]["plan_us"]["median"]
        row["ratio_per_sweep"] = row["weighted"]["us_per_sweep"] / row["unweighted"]["us_per_sweep"]
        out[name] = row
        print("200 x 200 %s: unweighted %.1f us in %d sweeps (status %d, clearance %s), weighted %.1f us in %d sweeps (status %d, clearance %s): "
              "ratio %.2f, per sweep %.2f"
              % (name, row["unweighted"]["plan_us"]["median"], row["unweighted"]["sweeps"], row["unweighted"]["status"],
                 row["unweighted"]["mean_clearance_cells"], row["weighted"]["plan_us"]["median"], row["weighted"]["sweeps"], row["weighted"]["status"],
                 row["weighted"]["mean_clearance_cells"], row["ratio"], row["ratio_per_sweep"]), file=sys.stderr, flush=True)
    return out


def resident_tick(ticks, rounds, warmup):
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(R, res)
    assert (warmup + ticks) * p.v_ref * p.dt / res < n // 2
    # a map's origin is a whole number of cells from (0, 0), its robot's start cell in its middle
    corner = np.floor(s0[:, :2] / res).astype(np.int64) - n // 2
    layers = [bs.layer(n, n, seed=20 + b) for b in range(B)]
    origins = [(corner[b, 0] * res, corner[b, 1] * res) for b in range(B)]
    occ = [(layers[b], origins[b], res, 0.0, 128) for b in range(B)]
    clear = [clearance_map(l) for l in layers]
    inst, map_of = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    goals = np.ascontiguousarray(np.tile(np.array([[n - 3, n - 3]], dtype=np.int32), (B, 1)))
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)
    last = {}

    def set_mode(h, mode):
        h.resident_set_paths(paths, res)   # (every round and mode from the fleet's own paths; the path's resolution is the map's)
        h.set_occupancy(occ, infl, map_of, W_GRID)
        h.resident_set_plan(CAPACITY, False)
        if mode == "plan_cost":
            h.resident_set_plan_penalty(GAIN, MAX_PENALTY)

    def after_step(mode, _i):
        if mode != "none":
            raw_plan(h, inst, goals, n * n + 1)

    def check(mode, kernel):
        bs.check_grid(mode, kernel)
        status, poses, _cell, _dist, sweeps = h.resident_read_plan()
        assert (status == 0).all() if mode == "none" else (status > 0).all(), status
        if mode != "none":
            c = [mean_clearance(clear[b], h.resident_read_path(b), origins[b], res) for b in range(B) if status[b] in (1, 2)]
            last[mode] = {"last_status": [int(s) for s in status], "last_sweeps": [int(s) for s in sweeps], "last_poses": [int(s) for s in poses],
                          "mean_sweeps": float(np.mean(sweeps)), "mean_clearance_cells": float(np.mean([v for v in c if v is not None])) if c else None}

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup,
                                             after_step=after_step, costmap_form=True, check=check)
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": R, "ticks": ticks, "warmup": warmup, "lethal": LETHAL, "capacity": CAPACITY,
           "gain": GAIN, "max_penalty": MAX_PENALTY, "plan_mode": "all %d robots plan after every tick, one call" % B, **last}
    h.close()
    bs.tick_stats(out, times, wall)
    for name in ("plan", "plan_cost"):
        out[name + "_tick_us"]["spread"] = float(max(times[name]) - min(times[name]))
    cost = lambda name: out[name + "_tick_us"]["median"] - out["none_tick_us"]["median"]
    out["plan_over_none_us"], out["plan_cost_over_none_us"] = cost("plan"), cost("plan_cost")
    out["ratio"] = cost("plan_cost") / cost("plan") if cost("plan") > 0 else None
    print("resident B=64 tick us (device events): none %.2f (spread %.2f)  plan %.2f  plan_cost %.2f; mean sweeps %.1f / %.1f; mean clearance %s / %s cells"
          % (out["none_tick_us"]["median"], out["none_tick_us"]["spread"], out["plan_tick_us"]["median"], out["plan_cost_tick_us"]["median"],
             last["plan"]["mean_sweeps"], last["plan_cost"]["mean_sweeps"], last["plan"]["mean_clearance_cells"], last["plan_cost"]["mean_clearance_cells"]),
          file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_plan_cost_timing.json", ticks=40, warmup=10).parse_args()
    out = {**bs.header(), "one_plan": one_plan(args.rounds), "resident": resident_tick(args.ticks, args.rounds, args.warmup)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

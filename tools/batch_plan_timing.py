#!/usr/bin/env python3
"""The device planner (ccv_mppi_batch_resident_plan_enqueue) against what a caller of the parent commit has
to do to give a resident fleet new paths: `python tools/batch_plan_timing.py [--out FILE]` (default
profiles/batch_plan_timing.json).  The method and the resident loop (its costmap form) are those of tools/bench_support.py.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 costmap per robot placed round its start pose at R = 6 (2 % of
the layer occupied): `none`, no planning; `plan`, all 64 robots plan after every tick, in one call, each to the far corner of
its own map.  Device events around --ticks ticks, us per tick, and the wall time of the same loop; `plan_call_us`, the host time
of one plan call of the 64 robots with the stream idle and a staging slot free.  `host_plan_ms`: the parent's only way, once per
round -- _resident_read (a flush and a synchronisation), _read_grid_cells of the 64 maps, the checker on the host
(tests/plan_reference.py: Dijkstra in Python, so this row is Python's speed, not a tuned planner's), _resident_set_paths.

One robot on one 200 x 200 float map -- empty, 3 % random, serpentine: `plan_us`, one plan call between two events, with the
sweeps it took and its status.  Nothing here asserts a time.  One JSON document goes to stdout (and --out)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(bs.ROOT, "tests"))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402
import plan_reference as PR  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
LETHAL = 0.8
TICK_MODES = ("none", "plan")
TICK_R, TICK_N, CAPACITY = 6, 200, 1024
i32p = C.POINTER(C.c_int32)


def raw_plan(h, inst, goals, max_sweeps):
    rc = h.lib.ccv_mppi_batch_resident_plan_enqueue(h._h, len(inst), inst.ctypes.data_as(i32p), goals.ctypes.data_as(i32p), LETHAL, max_sweeps)
    assert rc == capi.OK, rc


def resident_tick(ticks, rounds, warmup):
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(TICK_R, res)
    assert (warmup + ticks) * p.v_ref * p.dt / res < n // 2
    # a map's origin is a whole number of cells from (0, 0), its robot's start cell in its middle
    corner = np.floor(s0[:, :2] / res).astype(np.int64) - n // 2
    occ = [(bs.layer(n, n, seed=20 + b), (corner[b, 0] * res, corner[b, 1] * res), res, 0.0, 128) for b in range(B)]
    inst, map_of = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    goals = np.ascontiguousarray(np.tile(np.array([[n - 3, n - 3]], dtype=np.int32), (B, 1)))
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)

    def set_mode(h, _mode):
        h.resident_set_paths(paths, res)   # (every round and mode from the fleet's own paths; the path's resolution is the map's)
        h.set_occupancy(occ, infl, map_of, W_GRID)
        h.resident_set_plan(CAPACITY, False)

    def after_step(mode, _i):
        if mode == "plan":
            raw_plan(h, inst, goals, n * n + 1)

    def check(mode, kernel):
        bs.check_grid(mode, kernel)
        status = h.resident_read_plan()[0]
        assert (status == 0).all() if mode == "none" else (status > 0).all(), status

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup,
                                             after_step=after_step, costmap_form=True, check=check)
    status, poses, _cell, _dist, sweeps = h.resident_read_plan()
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks, "warmup": warmup, "lethal": LETHAL, "capacity": CAPACITY,
           "plan": "all %d robots plan after every tick, one call" % B,
           "last_status": [int(s) for s in status], "last_sweeps": [int(s) for s in sweeps], "last_poses": [int(s) for s in poses],
           "plan_call_us": bs.idle_call_us(h, lambda _i: raw_plan(h, inst, goals, n * n + 1), rounds)}

    # the parent's only way, once per round: read the poses and the cells back, plan on the host, install the paths
    def host_plan():
        pose = h.resident_read()[0]
        maps = h.get_grids()[0]
        new = []
        for b in range(B):
            r = PR.plan(maps[b][0], maps[b][1], res, pose[b, :2], goals[b], LETHAL, CAPACITY)
            new.append(r["path"] if r["path"] is not None else paths[b])
        h.resident_set_paths(new, res)

    host_ms = []
    for _ in range(rounds):
        set_mode(h, "none")
        h.resident_set_poses(s0, seeds)
        h.resident_step_enqueue(p.dt, 0, advance=False)
        host_ms.append(bs.wall_us(host_plan)[0] * 1e-3)
    out["host_plan_ms"] = bs.stats(host_ms)
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  plan %.2f / %.2f; one plan call of 64 robots %.2f us "
          "of host time; read-back, Python checker and _set_paths %.1f ms"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["plan_tick_us"]["median"],
             out["plan_wall_us"]["median"], out["plan_call_us"]["median"], out["host_plan_ms"]["median"]), file=sys.stderr, flush=True)
    return out


def one_plan(rounds):
    n, res = TICK_N, RESOLUTION
    p = configs.diff_drive_defaults(128, 15)
    kinds = {"empty": PR.empty(n, n), "random_0.03": np.where(np.random.default_rng(3).random((n, n)) < 0.03, 1.0, 0.0).astype(np.float32),
             "serpentine": PR.serpentine(n, n)}
    out = {"nx": n, "ny": n, "lethal": LETHAL}
    for name, cells in kinds.items():
        cells[0, 0] = 0.0
        goal = PR.free_cell(cells[::-1, ::-1], LETHAL, (0, 0))
        goals = np.array([[n - 1 - goal[0], n - 1 - goal[1]]], dtype=np.int32)
        if name == "serpentine":   # (half way up: the whole corridor is longer than the field can count)
            goals = np.array([[n // 2, n // 2]], dtype=np.int32)
        h = amd.BatchController(p, 1)
        stream = bs.new_stream()
        h.set_stream(stream.cuda_stream)
        h.resident_set_paths(amd.make_path("dkan"), res)
        h.resident_set_poses(np.array([[0.5 * res, 0.5 * res, 0.0]]), 1)
        h.set_grids([(cells, (0.0, 0.0), res, 0.0)], [0], W_GRID)
        h.resident_set_plan(capi.PLAN_MAX_POSES, False)
        inst = np.zeros(1, dtype=np.int32)
        raw_plan(h, inst, goals, n * n + 1)   # (warm-up)
        h.synchronize()
        ms, us = bs.one_call_ms_and_us(h, stream, rounds, lambda: raw_plan(h, inst, goals, n * n + 1))
        status, poses, _cell, dist, sweeps = h.resident_read_plan()
        h.close()
        out[name] = {"status": int(status[0]), "poses": int(poses[0]), "start_dist": int(dist[0]), "sweeps": int(sweeps[0]), "plan_ms": ms, "plan_us": us}
        print("200 x 200 %s: status %d, %d poses, %d sweeps, one plan %.1f us between two events"
              % (name, status[0], poses[0], sweeps[0], us["median"]), file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_plan_timing.json", ticks=40, warmup=10).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "one_plan": one_plan(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

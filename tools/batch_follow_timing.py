#!/usr/bin/env python3
"""Costmaps that follow their robots (ccv_mppi_batch_resident_follow_enqueue) against the parent commit's
only way to keep a window round a driving robot: `python tools/batch_follow_timing.py [--out FILE]` (default
profiles/batch_follow_bench.json).  The method and the resident loop (its costmap form) are those of tools/bench_support.py.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 map per robot round its start pose, R = 6: `none`, no map
change; `held`, all 64 maps followed after every tick with a margin no robot leaves, so every decision is HELD -- the cost of
the unconditional copy; `move`, all 64 followed with margin 0 and max_step 2, so every window moves with its robot (one or two
cells a tick at 0.8 m/s); `host`, the parent's way with the same margin and step: _resident_read (a flush and a
synchronisation), batch.follow_shift on the host, _roll_occupancy_enqueue; `read`, the _resident_read of that way alone, which
splits `host` into what any host-decided roll pays and what the decisions in the interpreter add.  Device events around
--ticks ticks, us per tick, and the wall time of the same loop; `follow_call_us`, the host time of one follow call of the 64
maps with the stream idle and a staging slot free.

One 4 000 x 3 000 map at R = 20 followed by 8 cells: `follow_ms`, the wall time of the call and a synchronisation,
`follow_kernels_us`, the two launches between two events, and the same two figures of the host-decided roll by 8 cells with
fill (`roll_ms`, `roll_kernels_us`).  One JSON document goes to stdout (and --out).  Nothing is asserted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, configs  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "held", "move", "read", "host")
TICK_R, TICK_N = 6, 200
BIG, BIG_R, BIG_DX = (4000, 3000), 20, 8
NEVER = 32768   # a margin no robot leaves (CCV_MPPI_GRID_MAX_DIM)


def resident_tick(ticks, rounds, warmup):
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(TICK_R, res)
    occ = [(bs.layer(n, n, seed=20 + b), (s0[b, 0] - 0.5 * n * res, s0[b, 1] - 0.5 * n * res), res, 0.0, 128) for b in range(B)]
    map_of = np.arange(B, dtype=np.int32)
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)

    def set_mode(h, mode):
        h.set_occupancy(occ, infl, map_of, W_GRID)   # (drops following; the windows are round the start poses again)
        h.roll_occupancy(map_of, 0, 0)               # (the priming call: the rolls below allocate nothing)
        if mode in ("held", "move"):
            h.resident_set_follow(True)

    def host_follow():
        st = h.resident_read()[0]
        geo = h.get_occupancy()
        d = np.concatenate([batch.follow_shift((geo[b][0], res, n, n), st[b:b + 1, :2], 0, 2) for b in range(B)])
        moved = np.flatnonzero(np.any(d != 0, axis=1)).astype(np.int32)
        if len(moved):
            h.roll_occupancy(moved, d[moved, 0], d[moved, 1], None, 0)

    def after_step(mode, _i):
        if mode == "held":
            h.resident_follow(map_of, NEVER, 1)
        elif mode == "move":
            h.resident_follow(map_of, 0, 2)
        elif mode == "read":
            h.resident_read()
        elif mode == "host":
            host_follow()

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup, None, after_step,
                                             costmap_form=True, check=bs.check_grid)
    h.set_occupancy(occ, infl, map_of, W_GRID)
    h.resident_set_follow(True)
    h.resident_set_poses(s0, seeds)
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks, "move": "margin 0, max_step 2, fill 0, one call for all maps",
           "follow_call_us": bs.idle_call_us(h, lambda _i: h.resident_follow(map_of, NEVER, 1), rounds)}
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): " + "  ".join("%s %.2f / %.2f (spread %.2f)" % (
        m, out[m + "_tick_us"]["median"], out[m + "_wall_us"]["median"], max(out[m + "_tick_us"]["rounds"]) - min(out[m + "_tick_us"]["rounds"]))
        for m in TICK_MODES)
        + "; one follow call of 64 maps %.2f us of host time" % out["follow_call_us"]["median"], file=sys.stderr, flush=True)
    return out


def big_map(rounds):
    nx, ny = BIG
    p = configs.diff_drive_defaults(128, 15)
    h = amd.BatchController(p, 1)
    infl = bs.inflation(BIG_R, RESOLUTION)
    occ = [(bs.layer(nx, ny), (0.0, 0.0), RESOLUTION, 0.0, 128)]
    stream = bs.new_stream()
    h.set_stream(stream.cuda_stream)
    paths, _s0, seeds = bs.fleet(p, 1)
    h.resident_set_paths(paths)
    centre = np.array([[(nx // 2 + 0.5) * RESOLUTION, (ny // 2 + 0.5) * RESOLUTION, 0.0]])
    h.set_occupancy(occ, infl, [0], W_GRID)
    h.roll_occupancy([0], 0, 0)
    one = np.zeros(1, dtype=np.int32)

    def roll(dx):
        h.roll_occupancy(one, dx, 0, None, 0)

    roll(BIG_DX), roll(-BIG_DX)   # (warm-up)
    h.synchronize()
    roll_ms, roll_us = bs.one_call_ms_and_us(h, stream, rounds, lambda: roll(BIG_DX), lambda: roll(-BIG_DX))   # (there, and back)
    # followed: the robot stands far right of the centre cell, so every call moves the window by max_step = 8 cells
    h.resident_set_follow(True)
    far = centre.copy()
    far[0, 0] += 1000.0 * BIG_DX * RESOLUTION
    h.resident_set_poses(far, seeds)
    h.resident_follow(one, 0, BIG_DX)   # (warm-up)
    h.synchronize()
    follow_ms, follow_us = bs.one_call_ms_and_us(h, stream, rounds, lambda: h.resident_follow(one, 0, BIG_DX))
    status = h.resident_read_follow()[0].tolist()
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "step": [BIG_DX, 0], "follow_ms": follow_ms, "follow_kernels_us": follow_us, "roll_ms": roll_ms,
           "roll_kernels_us": roll_us, "last_status": status}
    print("4000 x 3000 R=20 moved by (8, 0): followed, call and synchronisation %.3f ms, kernels %.1f us; host-decided roll %.3f ms, kernels %.1f us"
          % (follow_ms["median"], follow_us["median"], roll_ms["median"], roll_us["median"]), file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_follow_bench.json", ticks=256).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "big_map": big_map(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

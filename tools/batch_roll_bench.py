#!/usr/bin/env python3
"""Rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue) against what a caller of the parent commit has
to do when the windows move: `python tools/batch_roll_bench.py [--out FILE]` (default profiles/batch_roll_bench.json).  The method
and the resident loop (its costmap form) are those of tools/bench_support.py.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 map per robot, R = 6: `none`, no map change; `roll`, all 64
maps rolled by (1, 0) or (1, 1) cells with strips after every tick, in one call (the sign flips every eight ticks, so the windows
stay about where they were); `set_occupancy`, the parent's only way, a full _set_occupancy of the 64 moved maps before every tick
(layers precomputed: checks, upload, 64 inflations and the synchronisation are charged).  Device events around --ticks ticks, us
per tick, and the wall time of the same loop; `roll_call_us`, the host time of one roll call of the 64 maps with the stream idle
and a staging slot free.

One 4 000 x 3 000 map at R = 20 rolled by (8, 0) with its strip: `roll_ms`, the wall time of the call and a synchronisation,
`roll_kernels_us`, the two launches between two events, and `set_occupancy_ms`, a full _set_occupancy of it.  One JSON document
goes to stdout (and --out)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "roll", "set_occupancy")
TICK_R, TICK_N = 6, 200
BIG, BIG_R, BIG_DX = (4000, 3000), 20, 8
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def strips(sizes, dx, dy, seed):
    """the packed exposed buffer of one call: 2 % of the new cells occupied"""
    rng = np.random.default_rng(seed)
    n = sum(min(abs(b), ny) * nx + (ny - min(abs(b), ny)) * min(abs(a), nx) for (nx, ny), a, b in zip(sizes, dx, dy))
    return np.where(rng.random(n) < 0.02, 255, 0).astype(np.uint8)


def roll_args(B, n, phase):
    """(map, dx, dy, exposed) of one call: (1, 0) on even ticks and (1, 1) on odd ones, the sign by `phase`"""
    sign = 1 if phase < 8 else -1
    maps = np.arange(B, dtype=np.int32)
    dx = np.full(B, sign, dtype=np.int32)
    dy = np.full(B, sign * (phase % 2), dtype=np.int32)
    return maps, dx, dy, strips([(n, n)] * B, dx, dy, phase)


def raw_roll(h, maps, dx, dy, buf):
    rc = h.lib.ccv_mppi_batch_roll_occupancy_enqueue(h._h, len(maps), maps.ctypes.data_as(i32p), dx.ctypes.data_as(i32p), dy.ctypes.data_as(i32p),
                                                     buf.ctypes.data_as(u8p), 0)
    assert rc == capi.OK, rc


def resident_tick(ticks, rounds, warmup):
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(TICK_R, res)
    cells = [bs.layer(n, n, seed=20 + b) for b in range(B)]
    # (a window of 10 m centred on the robot's start; the moved variants of mode `set_occupancy` a cell apart)
    occ = [[(cells[b], (s0[b, 0] - 0.5 * n * res + k * res, s0[b, 1] - 0.5 * n * res), res, 0.0, 128) for b in range(B)] for k in range(4)]
    calls = [roll_args(B, n, phase) for phase in range(16)]
    map_of = np.arange(B, dtype=np.int32)
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)

    def set_mode(h, _mode):
        h.set_occupancy(occ[0], infl, map_of, W_GRID)
        h.roll_occupancy(map_of, 0, 0)   # (the priming call: the rolls below allocate nothing)

    def before_step(mode, i):
        if mode == "set_occupancy":
            h.set_occupancy(occ[i % 4], infl, map_of, W_GRID)

    def after_step(mode, i):
        if mode == "roll":
            raw_roll(h, *calls[i % 16])

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup, before_step,
                                             after_step, costmap_form=True, check=bs.check_grid)
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks,
           "roll": "(1, 0) and (1, 1) alternating, strips, one call for all maps",
           "roll_call_us": bs.idle_call_us(h, lambda i: raw_roll(h, *calls[i]), rounds)}
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  roll %.2f / %.2f  set_occupancy %.2f / %.2f; "
          "one roll call of 64 maps %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["roll_tick_us"]["median"],
             out["roll_wall_us"]["median"], out["set_occupancy_tick_us"]["median"], out["set_occupancy_wall_us"]["median"],
             out["roll_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def big_map(rounds):
    nx, ny = BIG
    h = amd.BatchController(configs.diff_drive_defaults(128, 15), 1)
    infl = bs.inflation(BIG_R, RESOLUTION)
    occ = [(bs.layer(nx, ny), (0.0, 0.0), RESOLUTION, 0.0, 128)]
    stream = bs.new_stream()
    h.set_stream(stream.cuda_stream)
    h.set_occupancy(occ, infl, [0], W_GRID)
    h.roll_occupancy([0], 0, 0)
    maps, dx, dy = np.zeros(1, dtype=np.int32), np.full(1, BIG_DX, dtype=np.int32), np.zeros(1, dtype=np.int32)
    buf = strips([BIG], dx, dy, 1)
    raw_roll(h, maps, dx, dy, buf)   # (warm-up)
    h.synchronize()
    roll_ms, kernels_us = bs.one_call_ms_and_us(h, stream, rounds, lambda: raw_roll(h, maps, dx, dy, buf),
                                                lambda: raw_roll(h, maps, -dx, dy, buf))   # (there, and back)
    full = [bs.wall_us(lambda: h.set_occupancy(occ, infl, [0], W_GRID))[0] * 1e-3 for _ in range(rounds)]
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "roll": [BIG_DX, 0], "roll_ms": roll_ms, "roll_kernels_us": kernels_us, "set_occupancy_ms": bs.stats(full, True)}
    print("4000 x 3000 R=20 rolled by (8, 0): call and synchronisation %.3f ms, kernels %.1f us; _set_occupancy %.2f ms (spread %.2f)"
          % (out["roll_ms"]["median"], out["roll_kernels_us"]["median"], out["set_occupancy_ms"]["median"], out["set_occupancy_ms"]["spread"]),
          file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_roll_bench.json", ticks=256).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "big_map": big_map(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

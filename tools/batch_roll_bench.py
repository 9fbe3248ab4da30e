#!/usr/bin/env python3
"""Rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue) against what a caller of the parent commit has
to do when the windows move: `python tools/batch_roll_bench.py [--out FILE]` (default profiles/batch_roll_bench.json).  The method
of tools/batch_costmap_bench.py: medians of --rounds rounds beside the max - min of the baseline's rounds.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 map per robot, R = 6: `none`, no map change; `roll`, all 64
maps rolled by (1, 0) or (1, 1) cells with strips after every tick, in one call (the sign flips every eight ticks, so the windows
stay about where they were); `set_occupancy`, the parent's only way, a full _set_occupancy of the 64 moved maps before every tick
(layers precomputed: checks, upload, 64 inflations and the synchronisation are charged).  Device events around --ticks ticks, us
per tick, and the wall time of the same loop; `roll_call_us`, the host time of one roll call of the 64 maps with the stream idle
and a staging slot free.

One 4 000 x 3 000 map at R = 20 rolled by (8, 0) with its strip: `roll_ms`, the wall time of the call and a synchronisation,
`roll_kernels_us`, the two launches between two events, and `set_occupancy_ms`, a full _set_occupancy of it.  One JSON document
goes to stdout (and --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402
from batch_costmap_bench import layer, stats  # noqa: E402
from batch_obstacles_bench import fleet  # noqa: E402

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
    import torch
    p, B, n = configs.diff_drive_defaults(1000, 15), 64, TICK_N
    paths, s0, seeds = fleet(p, B)
    res = RESOLUTION
    infl = batch.inflation_profile(TICK_R * res, res)
    assert infl[0] == TICK_R
    cells = [layer(n, n, seed=20 + b) for b in range(B)]
    # (a window of 10 m centred on the robot's start; the moved variants of mode `set_occupancy` a cell apart)
    occ = [[(cells[b], (s0[b, 0] - 0.5 * n * res + k * res, s0[b, 1] - 0.5 * n * res), res, 0.0, 128) for b in range(B)] for k in range(4)]
    calls = [roll_args(B, n, phase) for phase in range(16)]
    map_of = np.arange(B, dtype=np.int32)
    stream = torch.cuda.Stream()
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    times = {m: [] for m in TICK_MODES}
    wall = {m: [] for m in TICK_MODES}
    for _r in range(rounds):
        for mode in TICK_MODES:
            h.set_occupancy(occ[0], infl, map_of, W_GRID)
            h.roll_occupancy(map_of, 0, 0)   # (the priming call: the rolls below allocate nothing)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            h.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record(stream)
            for i in range(ticks):
                if mode == "set_occupancy":
                    h.set_occupancy(occ[i % 4], infl, map_of, W_GRID)
                h.resident_step_enqueue(p.dt, warmup + i)
                if mode == "roll":
                    raw_roll(h, *calls[i % 16])
            stop.record(stream)
            stop.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e6 / ticks)
            times[mode].append(start.elapsed_time(stop) * 1e3 / ticks)
            assert h.last_kernel() & capi.BATCH_KERNEL_GRID
    # the host time of the call itself: stream idle, slots free (fewer calls than slots between two synchronisations)
    call = []
    for _r in range(8 * rounds):
        h.synchronize()
        t0 = time.perf_counter()
        for i in range(capi.OCC_PATCH_SLOTS - 1):
            raw_roll(h, *calls[i])
        call.append((time.perf_counter() - t0) * 1e6 / (capi.OCC_PATCH_SLOTS - 1))
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks,
           "roll": "(1, 0) and (1, 1) alternating, strips, one call for all maps"}
    out["roll_call_us"] = stats(call[rounds:])
    for mode in TICK_MODES:
        out[mode + "_tick_us"] = stats(times[mode], mode == "none")
        out[mode + "_wall_us"] = stats(wall[mode], mode == "none")
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  roll %.2f / %.2f  set_occupancy %.2f / %.2f; "
          "one roll call of 64 maps %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["roll_tick_us"]["median"],
             out["roll_wall_us"]["median"], out["set_occupancy_tick_us"]["median"], out["set_occupancy_wall_us"]["median"],
             out["roll_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def big_map(rounds):
    import torch
    nx, ny = BIG
    h = amd.BatchController(configs.diff_drive_defaults(128, 15), 1)
    infl = batch.inflation_profile(BIG_R * RESOLUTION, RESOLUTION)
    assert infl[0] == BIG_R
    occ = [(layer(nx, ny), (0.0, 0.0), RESOLUTION, 0.0, 128)]
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    h.set_occupancy(occ, infl, [0], W_GRID)
    h.roll_occupancy([0], 0, 0)
    maps, dx, dy = np.zeros(1, dtype=np.int32), np.full(1, BIG_DX, dtype=np.int32), np.zeros(1, dtype=np.int32)
    buf = strips([BIG], dx, dy, 1)
    raw_roll(h, maps, dx, dy, buf)   # (warm-up)
    h.synchronize()
    roll, kern, full = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        raw_roll(h, maps, dx, dy, buf)
        h.synchronize()
        roll.append((time.perf_counter() - t0) * 1e3)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        raw_roll(h, maps, -dx, dy, buf)
        stop.record(stream)
        stop.synchronize()
        kern.append(start.elapsed_time(stop) * 1e3)
    for _ in range(rounds):
        t0 = time.perf_counter()
        h.set_occupancy(occ, infl, [0], W_GRID)
        full.append((time.perf_counter() - t0) * 1e3)
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "roll": [BIG_DX, 0], "roll_ms": stats(roll), "roll_kernels_us": stats(kern),
           "set_occupancy_ms": stats(full, True)}
    print("4000 x 3000 R=20 rolled by (8, 0): call and synchronisation %.3f ms, kernels %.1f us; _set_occupancy %.2f ms (spread %.2f)"
          % (out["roll_ms"]["median"], out["roll_kernels_us"]["median"], out["set_occupancy_ms"]["median"], out["set_occupancy_ms"]["spread"]),
          file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_roll_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "cus": props.multi_processor_count, "resident": resident_tick(args.ticks, args.rounds, args.warmup),
           "big_map": big_map(args.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

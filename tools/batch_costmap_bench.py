#!/usr/bin/env python3
"""Costmaps inflated on the device (ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue) against what a
caller of the parent commit has to do: `python tools/batch_costmap_bench.py [--out FILE]` (default
profiles/batch_costmap_bench.json).  The method of tools/batch_obstacles_bench.py: medians of --rounds rounds beside the
max - min of the baseline's rounds.

Full inflation, 400 x 300 and 4 000 x 3 000 cells at R = 3 and R = 20, 2 % of the cells occupied: `device_ms`, the wall time of
one _set_occupancy (checks, allocation, upload of the uint8 layer, one k_inflate launch, synchronisation); `host_ms`, the
baseline: the numpy checker (tests/costmap_reference.py, the separable form) on the host plus one _set_grids with its float map;
`kernels_us` (400 x 300 only: a whole-map patch is within CCV_MPPI_OCC_PATCH_MAX_CELLS), the patch writer and k_inflate over the
whole map between two events.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 400 x 300 map shared by all instances, R = 6: `none`, no map updates;
`patch`, one 64 x 64 patch enqueued after every tick; `patch_1x1`, a patch of one cell (the floor: two more launches of one workgroup
each); `set_grids`, the parent's only way, a full _set_grids before every tick
(the map itself precomputed: only the upload is charged).  Device events around --ticks ticks, us per tick, and the wall
time of the same loop; `patch_call_us`, the host time of one _update_occupancy_enqueue call with the stream idle and a staging slot
free (what the call costs the thread that makes it).  One JSON document goes to stdout (and --out)."""
import argparse
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
import costmap_reference as CR  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402
from batch_obstacles_bench import fleet  # noqa: E402

SIZES = ((400, 300), (4000, 3000))
RADII = (3, 20)
RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "patch", "patch_1x1", "set_grids")
TICK_R, PATCH = 6, 64


def layer(nx, ny, seed=9):
    return np.where(np.random.default_rng(seed).random((ny, nx)) < 0.02, 255, 0).astype(np.uint8)


def stats(v, baseline=False):
    out = {"median": float(np.median(v)), "rounds": [float(x) for x in v]}
    if baseline:
        out["spread"] = float(max(v) - min(v))
    return out


def full_inflation(rounds):
    import torch
    h = amd.BatchController(configs.diff_drive_defaults(128, 15), 1)
    out = []
    for nx, ny in SIZES:
        cells = layer(nx, ny)
        for R in RADII:
            infl = batch.inflation_profile(R * RESOLUTION, RESOLUTION)
            assert infl[0] == R
            occ = [(cells, (0.0, 0.0), RESOLUTION, 0.0, 128)]
            h.set_occupancy(occ, infl, [0], W_GRID)   # (warm-up)
            dev, host, kern = [], [], []
            for _ in range(rounds):
                t0 = time.perf_counter()
                h.set_occupancy(occ, infl, [0], W_GRID)
                dev.append((time.perf_counter() - t0) * 1e3)
                if nx * ny <= capi.OCC_PATCH_MAX_CELLS:
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream = torch.cuda.Stream()
                    h.set_stream(stream.cuda_stream)
                    start.record(stream)
                    h.update_occupancy(0, 0, 0, cells)
                    stop.record(stream)
                    stop.synchronize()
                    h.set_stream(0)
                    kern.append(start.elapsed_time(stop) * 1e3)
            got = h.get_grids()[0][0][0]
            for _ in range(rounds):
                t0 = time.perf_counter()
                cost = CR.cost_separable(cells, 128, *infl)
                h.set_grids([(cost, (0.0, 0.0), RESOLUTION, 0.0)], [0], W_GRID)
                host.append((time.perf_counter() - t0) * 1e3)
            assert got.tobytes() == cost.tobytes()
            r = {"nx": nx, "ny": ny, "R": R, "device_ms": stats(dev), "host_ms": stats(host, True)}
            if kern:
                r["kernels_us"] = stats(kern)
            out.append(r)
            print("inflation %4d x %4d R=%2d: device %.2f ms, host %.1f ms (spread %.1f)%s"
                  % (nx, ny, R, r["device_ms"]["median"], r["host_ms"]["median"], r["host_ms"]["spread"],
                     ", kernels %.1f us" % r["kernels_us"]["median"] if kern else ""), file=sys.stderr, flush=True)
    h.close()
    return out


def resident_tick(ticks, rounds, warmup):
    import torch
    p, B = configs.diff_drive_defaults(1000, 15), 64
    nx, ny = SIZES[0]
    paths, s0, seeds = fleet(p, B)
    xs, ys = np.concatenate([q[0] for q in paths]), np.concatenate([q[1] for q in paths])
    lo_x, hi_x, lo_y, hi_y = float(xs.min()) - 3.0, float(xs.max()) + 3.0, float(ys.min()) - 3.0, float(ys.max()) + 3.0
    res = max((hi_x - lo_x) / nx, (hi_y - lo_y) / ny)
    cells = layer(nx, ny)
    infl = batch.inflation_profile(TICK_R * res, res)
    assert infl[0] == TICK_R
    cost = CR.cost_separable(cells, 128, *infl)
    rng = np.random.default_rng(3)
    patches = [(int(rng.integers(0, nx - PATCH)), int(rng.integers(0, ny - PATCH)), np.where(rng.random((PATCH, PATCH)) < 0.02, 255, 0).astype(np.uint8))
               for _ in range(16)]
    one = np.full((1, 1), 255, dtype=np.uint8)
    stream = torch.cuda.Stream()
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    times = {m: [] for m in TICK_MODES}
    wall = {m: [] for m in TICK_MODES}
    for _r in range(rounds):
        for mode in TICK_MODES:
            if mode == "set_grids":
                h.set_grids([(cost, (lo_x, lo_y), res, 0.0)], 0, W_GRID)
            else:
                h.set_occupancy([(cells, (lo_x, lo_y), res, 0.0, 128)], infl, 0, W_GRID)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            h.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record(stream)
            for i in range(ticks):
                if mode == "set_grids":
                    h.set_grids([(cost, (lo_x, lo_y), res, 0.0)], 0, W_GRID)
                h.resident_step_enqueue(p.dt, warmup + i)
                if mode == "patch":
                    h.update_occupancy(0, *patches[i % len(patches)])
                elif mode == "patch_1x1":
                    h.update_occupancy(0, patches[i % len(patches)][0], patches[i % len(patches)][1], one)
            stop.record(stream)
            stop.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e6 / ticks)
            times[mode].append(start.elapsed_time(stop) * 1e3 / ticks)
            assert h.last_kernel() & capi.BATCH_KERNEL_GRID
    # the host time of the call itself: stream idle, slots free (fewer calls than slots between two synchronisations)
    h.set_occupancy([(cells, (lo_x, lo_y), res, 0.0, 128)], infl, 0, W_GRID)
    call = []
    for _r in range(8 * rounds):
        h.synchronize()
        t0 = time.perf_counter()
        for i in range(capi.OCC_PATCH_SLOTS - 1):
            h.update_occupancy(0, *patches[i])
        call.append((time.perf_counter() - t0) * 1e6 / (capi.OCC_PATCH_SLOTS - 1))
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "map": [nx, ny], "R": TICK_R, "patch": [PATCH, PATCH], "ticks": ticks}
    out["patch_call_us"] = stats(call[rounds:])
    for mode in TICK_MODES:
        out[mode + "_tick_us"] = stats(times[mode], mode == "none")
        out[mode + "_wall_us"] = stats(wall[mode], mode == "none")
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  patch %.2f / %.2f  patch 1 x 1 %.2f / %.2f  "
          "set_grids %.2f / %.2f; one patch call %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["patch_tick_us"]["median"],
             out["patch_wall_us"]["median"], out["patch_1x1_tick_us"]["median"], out["patch_1x1_wall_us"]["median"],
             out["set_grids_tick_us"]["median"], out["set_grids_wall_us"]["median"], out["patch_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_costmap_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "cus": props.multi_processor_count, "resident": resident_tick(args.ticks, args.rounds, args.warmup),
           "inflation": full_inflation(args.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The occupancy-grid form of the batch handles' rollout kernels (ccv_mppi_batch_set_grids) against the moving-disc form on the
same handle, same process, same inputs: `python tools/batch_grid_bench.py [--out FILE]` (default
profiles/batch_grid_bench.json).  The method of tools/batch_obstacles_bench.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters on the inputs of
tools/batch_params_bench.py and n = 8 moving discs per instance (weight 1, scattered within 3 m of the window, up to 1.5 m/s).
Three modes alternate on that handle round by round (--rounds): `off`, the MOVING kernels; `small`, the GRID kernels over one
400 x 300 map shared by all instances (480 KB); `large`, over one 4 000 x 3 000 map (48 MB, larger than the L2).  Both maps
cover the bounding box of all windows plus 3 m, so nearly every state is in bounds; the cells are random.  Each round is the
mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the rollout kernel, *_iter_us the whole
launch sequence, medians over the rounds, and spread_off_* = max - min of the off rounds.  The yardstick is the off kernel of
the same run.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident closed loop (device events over --ticks ticks, us
per tick), the same three modes.  One JSON document goes to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402
from batch_params_bench import inputs  # noqa: E402
from batch_shift_bench import times_us  # noqa: E402
from batch_obstacles_bench import fleet, scatter  # noqa: E402
from batch_moving_bench import velocities  # noqa: E402

N_DISCS = 8
SIZES = {"small": (400, 300), "large": (4000, 3000)}
MODES = ("off", "small", "large")
W_GRID = 0.01


def maps_over(xs, ys, seed=9):
    """{name: (cells, origin, resolution, outside)} over the bounding box of the points plus 3 m"""
    lo_x, hi_x, lo_y, hi_y = float(np.min(xs)) - 3.0, float(np.max(xs)) + 3.0, float(np.min(ys)) - 3.0, float(np.max(ys)) + 3.0
    rng = np.random.default_rng(seed)
    out = {}
    for name, (nx, ny) in SIZES.items():
        res = max((hi_x - lo_x) / nx, (hi_y - lo_y) / ny)
        out[name] = (rng.random((ny, nx), dtype=np.float32), (lo_x, lo_y), res, 1.0)
    return out


def set_mode(h, maps, mode):
    h.set_grids(None if mode == "off" else [maps[mode]], 0, W_GRID)


def summarise(res, times, unit):
    for k, v in times.items():
        res[k + unit] = float(np.median(v))
        if k.startswith("off"):
            res["spread_" + k + unit] = float(max(v) - min(v))


def measure(p, B, iters, rounds, warmup):
    ins = inputs(p, B)
    centres = np.stack([ins[2][:, p.horizon // 2], ins[3][:, p.horizon // 2]], axis=1)   # (x_ref, y_ref of the windows)
    maps = maps_over(ins[2], ins[3])
    h = amd.BatchController([p] * B, B)
    h.set_obstacles(scatter(centres, N_DISCS), 1.0, velocities=velocities(B, N_DISCS))
    for mode in MODES:
        set_mode(h, maps, mode)
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {m + s: [] for m in MODES for s in ("_kernel", "_iter")}
    kernel = {}
    for r in range(rounds):
        for mode in MODES:
            set_mode(h, maps, mode)
            k, t = times_us(h, ins, iters, r * iters)
            times[mode + "_kernel"].append(k)
            times[mode + "_iter"].append(t)
            kernel[mode] = h.last_kernel()
            assert bool(kernel[mode] & capi.BATCH_KERNEL_GRID) == (mode != "off") and kernel[mode] & capi.BATCH_KERNEL_MOVING
    h.close()
    res = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "discs": N_DISCS, "kernel": kernel, "rounds": rounds,
           "iters_per_round": iters, "per_round": {k + "_us": v for k, v in times.items()}}
    summarise(res, times, "_us")
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    import torch
    paths, s0, seeds = fleet(p, B)
    maps = maps_over(np.concatenate([q[0] for q in paths]), np.concatenate([q[1] for q in paths]))
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.set_obstacles(scatter(s0[:, :2], N_DISCS), 1.0, velocities=velocities(B, N_DISCS))
    h.resident_set_paths(paths)
    times = {m + "_tick": [] for m in MODES}
    kernel = {}
    for _r in range(rounds):
        for mode in MODES:
            set_mode(h, maps, mode)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for i in range(ticks):
                h.resident_step_enqueue(p.dt, warmup + i)
            stop.record(stream)
            stop.synchronize()
            times[mode + "_tick"].append(start.elapsed_time(stop) * 1e3 / ticks)
            kernel[mode] = h.last_kernel()
            assert bool(kernel[mode] & capi.BATCH_KERNEL_GRID) == (mode != "off")
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "discs": N_DISCS, "ticks": ticks, "rounds": rounds,
           "kernel": kernel, "per_round": {k + "_us": v for k, v in times.items()}}
    summarise(out, times, "_us")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=256, help="timed launches per round (>= 256)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_grid_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {"device": props.name, "cus": props.multi_processor_count, "maps": {k: list(v) for k, v in SIZES.items()}, "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f (spread %.2f)  small %7.2f  large %7.2f   iter us: off %7.2f small %7.2f large %7.2f"
              % (p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["spread_off_kernel_us"], r["small_kernel_us"],
                 r["large_kernel_us"], r["off_iter_us"], r["small_iter_us"], r["large_iter_us"]), file=sys.stderr, flush=True)
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, torch.cuda.Stream())
    out["resident"] = r
    print("resident B=64 tick us: off %.2f (spread %.2f)  small %.2f  large %.2f"
          % (r["off_tick_us"], r["spread_off_tick_us"], r["small_tick_us"], r["large_tick_us"]), file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

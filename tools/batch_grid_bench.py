#!/usr/bin/env python3
"""The occupancy-grid form of the batch handles' rollout kernels (ccv_mppi_batch_set_grids) against the moving-disc form on the
same handle, same process, same inputs: `python tools/batch_grid_bench.py [--out FILE]` (default
profiles/batch_grid_bench.json).  The method, the inputs and both loops are those of tools/bench_support.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters and n = 8 moving discs per instance
(weight 1, scattered within 3 m of the window, up to 1.5 m/s).
Three modes alternate on that handle round by round (--rounds): `off`, the MOVING kernels; `small`, the GRID kernels over one
400 x 300 map shared by all instances (480 KB); `large`, over one 4 000 x 3 000 map (48 MB, larger than the L2).  Both maps
cover the bounding box of all windows plus 3 m, so nearly every state is in bounds; the cells are random.  Each round is the
mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the rollout kernel, *_iter_us the whole
launch sequence, medians over the rounds, and spread_off_* = max - min of the off rounds.  The yardstick is the off kernel of
the same run.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident closed loop (device events over --ticks ticks, us
per tick), the same three modes.  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

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


def mode_setter(maps):
    return lambda h, mode: h.set_grids(None if mode == "off" else [maps[mode]], 0, W_GRID)


def measure(p, B, iters, rounds, warmup):
    ins = bs.inputs(p, B)
    h = amd.BatchController([p] * B, B)
    h.set_obstacles(bs.scatter(bs.window_centres(p, ins), N_DISCS), 1.0, velocities=bs.velocities(B, N_DISCS))

    def check(mode, kernel):
        assert bool(kernel & capi.BATCH_KERNEL_GRID) == (mode != "off") and kernel & capi.BATCH_KERNEL_MOVING

    times, kernel = bs.measure_modes(h, ins, MODES, mode_setter(maps_over(ins[2], ins[3])), iters, rounds, warmup, check=check)
    h.close()
    res = {**bs.shape(p, B), "discs": N_DISCS, "kernel": kernel, "rounds": rounds, "iters_per_round": iters}
    bs.summary(res, times, "_us")
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    paths, s0, seeds = bs.fleet(p, B)
    maps = maps_over(np.concatenate([q[0] for q in paths]), np.concatenate([q[1] for q in paths]))
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.set_obstacles(bs.scatter(s0[:, :2], N_DISCS), 1.0, velocities=bs.velocities(B, N_DISCS))
    h.resident_set_paths(paths)

    def check(mode, kernel):
        assert bool(kernel & capi.BATCH_KERNEL_GRID) == (mode != "off")

    times, _wall, kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, MODES, mode_setter(maps), ticks, rounds, warmup, check=check)
    h.close()
    out = {**bs.shape(p, B), "discs": N_DISCS, "ticks": ticks, "rounds": rounds, "kernel": kernel}
    bs.summary(out, times, "_tick_us")
    return out


def main():
    args = bs.parser("batch_grid_bench.json", iters=256, ticks=256).parse_args()
    out = {**bs.header(), "maps": {k: list(v) for k, v in SIZES.items()}, "configs": []}
    for p, B in bs.varied_plan():
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f (spread %.2f)  small %7.2f  large %7.2f   iter us: off %7.2f small %7.2f large %7.2f"
              % (p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["spread_off_kernel_us"], r["small_kernel_us"],
                 r["large_kernel_us"], r["off_iter_us"], r["small_iter_us"], r["large_iter_us"]), file=sys.stderr, flush=True)
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, bs.new_stream())
    out["resident"] = r
    print("resident B=64 tick us: off %.2f (spread %.2f)  small %.2f  large %.2f"
          % (r["off_tick_us"], r["spread_off_tick_us"], r["small_tick_us"], r["large_tick_us"]), file=sys.stderr, flush=True)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

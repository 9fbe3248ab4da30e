#!/usr/bin/env python3
"""The moving-disc form of the batch handles' obstacle term (ccv_mppi_batch_set_obstacle_velocities) against the static form on
the same handle, same process, same inputs: `python tools/batch_moving_bench.py [--out FILE]` (default
profiles/batch_moving_bench.json).  The method of tools/batch_obstacles_bench.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters on the inputs of
tools/batch_params_bench.py and n = 8 and n = 32 discs per instance (weight 1, scattered within 3 m of the window); per n the
static OBST kernels (no velocity table) and the MOVING kernels (velocities of up to 1.5 m/s) alternate on that handle round by
round (--rounds), each round the mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the
rollout kernel, *_iter_us the whole launch sequence, medians over the rounds, and spread_static_* = max - min of the static
rounds.  The yardstick is the static kernel of the same run.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident closed
loop with the fleet term (tools/batch_fleet_bench.py's fleet: max_neighbours = 4 and 16 under a range that holds every robot),
prediction off against on, alternating round by round (device events over --ticks ticks, us per tick, spread of the off
rounds).  One JSON document goes to stdout (and --out)."""
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

NS = (8, 32)
MODES = [("static_n%d" % n, n, False) for n in NS] + [("moving_n%d" % n, n, True) for n in NS]
MODES.sort(key=lambda m: m[1])   # static n8, moving n8, static n32, moving n32


def velocities(B, n, seed=6):
    return list(np.random.default_rng(seed).uniform(-1.5, 1.5, (B, n, 2)))


def set_mode(h, discs, vels, n, moving):
    h.set_obstacles(discs[n], 1.0, velocities=vels[n] if moving else None)


def measure(p, B, iters, rounds, warmup):
    ins = inputs(p, B)
    centres = np.stack([ins[2][:, p.horizon // 2], ins[3][:, p.horizon // 2]], axis=1)   # (x_ref, y_ref of the windows)
    discs = {n: scatter(centres, n) for n in NS}
    vels = {n: velocities(B, n) for n in NS}
    h = amd.BatchController([p] * B, B)
    for _name, n, moving in MODES:
        set_mode(h, discs, vels, n, moving)
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {m + s: [] for m, _, _ in MODES for s in ("_kernel", "_iter")}
    kernel = {}
    for r in range(rounds):
        for name, n, moving in MODES:
            set_mode(h, discs, vels, n, moving)
            k, t = times_us(h, ins, iters, r * iters)
            times[name + "_kernel"].append(k)
            times[name + "_iter"].append(t)
            kernel[name] = h.last_kernel()
            assert bool(kernel[name] & capi.BATCH_KERNEL_MOVING) == moving
    h.close()
    res = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "kernel": kernel, "rounds": rounds,
           "iters_per_round": iters, "per_round": {k + "_us": v for k, v in times.items()}}
    for k, v in times.items():
        res[k + "_us"] = float(np.median(v))
        if k.startswith("static"):
            res["spread_" + k + "_us"] = float(max(v) - min(v))
    return res


def resident_prediction(p, B, ticks, rounds, warmup, stream, neighbours=(4, 16), radius=0.3, reach=1.0e3):
    import torch
    paths, s0, seeds = fleet(p, B)
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    modes = [(("pred%d" if on else "off%d") % m, on, m) for m in neighbours for on in (False, True)]
    times = {name + "_tick": [] for name, _, _ in modes}
    kernel = {}
    for _r in range(rounds):
        for name, on, m in modes:
            h.resident_set_fleet(radius, reach, m, 1.0)
            h.resident_set_fleet_prediction(on)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for i in range(ticks):
                h.resident_step_enqueue(p.dt, warmup + i)
            stop.record(stream)
            stop.synchronize()
            times[name + "_tick"].append(start.elapsed_time(stop) * 1e3 / ticks)
            kernel[name] = h.last_kernel()
            assert bool(kernel[name] & capi.BATCH_KERNEL_MOVING) == on
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "rounds": rounds, "kernel": kernel,
           "per_round": {k + "_us": v for k, v in times.items()}}
    for k, v in times.items():
        out[k + "_us"] = float(np.median(v))
        if k.startswith("off"):
            out["spread_" + k + "_us"] = float(max(v) - min(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=256, help="timed launches per round (>= 256)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_moving_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {"device": props.name, "cus": props.multi_processor_count, "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: n8 static %7.2f moving %7.2f (static spread %.2f)  n32 static %7.2f moving %7.2f "
              "(static spread %.2f)" % (p.model, p.num_samples, p.horizon, B, r["static_n8_kernel_us"], r["moving_n8_kernel_us"],
                                        r["spread_static_n8_kernel_us"], r["static_n32_kernel_us"], r["moving_n32_kernel_us"],
                                        r["spread_static_n32_kernel_us"]), file=sys.stderr, flush=True)
    r = resident_prediction(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, torch.cuda.Stream())
    out["resident_fleet"] = r
    print("resident fleet B=64 tick us: " + "  ".join("%s %.2f" % (k[:-3], v) for k, v in r.items() if k.endswith("_tick_us")),
          file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fleet term of batch handles (ccv_mppi_batch_resident_set_fleet) against the same handle with the term off, same process,
same poses: `python tools/batch_fleet_bench.py [--out FILE]` (default profiles/batch_fleet_bench.json).

The resident tick (device events over --ticks ticks, us per tick) of ONE handle per configuration: diff drive K = 1 000, H = 15
at B = 8, 64, 256 and full body K = 10 000, H = 15 at B = 4.  For max_neighbours m in {4, 16} two modes alternate round by
round (--rounds): "off" = the term off with m static discs per robot, scattered within 3 m of its start, so that the same
rollout kernel does the same loop work, and "on" = the term on with max_neighbours = m and a range that holds every robot.
Medians over the rounds, and spread_* = max - min of the off rounds: the yardstick is the off mode of the same run.
`--trace` runs one short on-mode loop per configuration and nothing else, for a kernel-trace run of its own
(rocprofv3 --kernel-trace --stats -- python tools/batch_fleet_bench.py --trace): the k_finalize_advance_batch* time is read
from its statistics.  One JSON document goes to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402
from batch_obstacles_bench import fleet, scatter  # noqa: E402
from batch_shift_bench import summary  # noqa: E402

NEIGHBOURS = (4, 16)
RADIUS, WEIGHT, RANGE = 0.3, 1.0, 1.0e3


def set_mode(h, on, m, discs):
    if on:
        h.set_obstacles(None)
        h.resident_set_fleet(RADIUS, RANGE, m, WEIGHT)
    else:
        h.resident_set_fleet(None)
        h.set_obstacles(discs[m], WEIGHT)


def resident_tick(p, B, ticks, rounds, warmup, stream, trace=False):
    import torch
    paths, s0, seeds = fleet(p, B)
    discs = {m: scatter(s0[:, :2], m) for m in NEIGHBOURS}
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    modes = [("on%d" % m, True, m) for m in NEIGHBOURS] if trace else \
            [(("on%d" if on else "off%d") % m, on, m) for m in NEIGHBOURS for on in (False, True)]
    times = {name + "_tick": [] for name, _, _ in modes}
    kernel = {}
    for _r in range(1 if trace else rounds):
        for name, on, m in modes:
            set_mode(h, on, m, discs)
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
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "rounds": rounds, "kernel": kernel,
           "per_round": {k + "_us": v for k, v in times.items()}}
    summary(out, times, "_us")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--trace", action="store_true", help="one short on-mode loop per configuration, for a kernel-trace run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fleet_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (8, 64, 256)] + [(configs.full_body_defaults(10000, 15), 4)]
    out = {"device": props.name, "cus": props.multi_processor_count, "radius_m": RADIUS, "range_m": RANGE, "resident": []}
    stream = torch.cuda.Stream()
    for p, B in plan:
        r = resident_tick(p, B, 64 if args.trace else args.ticks, args.rounds, args.warmup, stream, args.trace)
        out["resident"].append(r)
        print("%-12s K=%6d B=%4d tick us: %s" % (p.model, p.num_samples, B, "  ".join(
            "%s %.2f" % (k[:-3], v) for k, v in r.items() if k.endswith("_tick_us"))), file=sys.stderr, flush=True)
    if args.trace:
        return
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

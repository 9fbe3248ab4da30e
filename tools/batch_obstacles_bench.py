#!/usr/bin/env python3
"""The disc-obstacle term of batch handles (ccv_mppi_batch_set_obstacles) against the same handle with the term off, same
process, same inputs: `python tools/batch_obstacles_bench.py [--out FILE]` (default profiles/batch_obstacles_bench.json).

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters (B copies of the configuration: the
obstacle-off VARIED kernel is the yardstick) on the inputs of tools/batch_params_bench.py; the term off, on with n = 8 and on
with n = 32 discs per instance (weight 1, scattered within 3 m of the window) alternate on that handle round by round
(--rounds), each round the mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the rollout
kernel, *_iter_us the whole launch sequence, medians over the rounds, and spread_* = max - min of the off rounds.  Diff drive
K = 1 000, H = 15, B = 64 also runs the resident closed loop the same way (device events over --ticks ticks, us per tick).
The behavioural leg: 64 robots on the sinusoid path, shifted weights on, each with one disc (r = 0.4 m, weight 200) centred on
a path point ahead; per robot the smallest distance of its trace to the disc's centre with the term off and on, and the RMS
distance to the path.  One JSON document goes to stdout (and --out)."""
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
from batch_params_bench import inputs, tracking_errors  # noqa: E402
from batch_shift_bench import times_us, summary  # noqa: E402

MODES = (("off", 0), ("n8", 8), ("n32", 32))


def scatter(centres, n, seed=5):
    """n discs per instance within 3 m of `centres` [B][2], radius 0.2 .. 0.5 m"""
    rng = np.random.default_rng(seed)
    B = len(centres)
    d = np.zeros((B, n, 3))
    d[:, :, :2] = np.asarray(centres)[:, None, :] + rng.uniform(-3.0, 3.0, (B, n, 2))
    d[:, :, 2] = rng.uniform(0.2, 0.5, (B, n))
    return list(d)


def set_mode(h, discs, n):
    h.set_obstacles(discs[n] if n else None, 1.0)


def measure(p, B, iters, rounds, warmup):
    ins = inputs(p, B)
    centres = np.stack([ins[2][:, p.horizon // 2], ins[3][:, p.horizon // 2]], axis=1)   # (x_ref, y_ref of the windows)
    discs = {n: scatter(centres, n) for _, n in MODES if n}
    h = amd.BatchController([p] * B, B)
    for _name, n in MODES:
        set_mode(h, discs, n)
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {m + s: [] for m, _ in MODES for s in ("_kernel", "_iter")}
    kernel = {}
    for r in range(rounds):
        for name, n in MODES:
            set_mode(h, discs, n)
            k, t = times_us(h, ins, iters, r * iters)
            times[name + "_kernel"].append(k)
            times[name + "_iter"].append(t)
            kernel[name] = h.last_kernel()
    h.close()
    res = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "kernel": kernel, "rounds": rounds,
           "iters_per_round": iters, "per_round": {k + "_us": v for k, v in times.items()}}
    summary(res, times, "_us")
    return res


def fleet(p, B):
    kinds = [amd.make_path("sinusoid", length=40.0), amd.make_path("dkan")]
    paths = [kinds[b % 2] for b in range(B)]
    s0 = np.zeros((B, p.nstate))
    for b in range(B):
        px, py = paths[b]
        i = (13 * b) % (len(px) // 4)
        s0[b, 0], s0[b, 1] = px[i], py[i] + 0.02 * ((b % 5) - 2)
        s0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
    return paths, s0, np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)


def resident_tick(p, B, ticks, rounds, warmup, stream):
    import torch
    paths, s0, seeds = fleet(p, B)
    discs = {n: scatter(s0[:, :2], n) for _, n in MODES if n}
    h = amd.BatchController([p] * B, B)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    times = {m + "_tick": [] for m, _ in MODES}
    kernel = {}
    for _r in range(rounds):
        for name, n in MODES:
            set_mode(h, discs, n)
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


def behaviour(ticks, B=64, radius=0.4, weight=200.0):
    p = configs.diff_drive_defaults(1000, 15)
    px, py = amd.make_path("sinusoid", length=40.0)
    s0 = np.zeros((B, 3))
    discs = []
    for b in range(B):
        i = (5 * b) % (len(px) // 4)
        s0[b] = (px[i], py[i], np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]))
        j = i + 40 + (b % 7)
        discs.append(np.array([[px[j], py[j], radius]]))
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)
    robots = [{"disc": [float(v) for v in discs[b][0]]} for b in range(B)]
    for name, on in (("off", False), ("on", True)):
        bat = amd.BatchController(p, B, min_shift=True)
        if on:
            bat.set_obstacles(discs, weight)
        bat.resident_set_paths((px, py))
        bat.resident_set_poses(s0, seeds)
        for i in range(ticks):
            bat.resident_step_enqueue(p.dt, i, advance=i > 0)
        bat.synchronize()
        for b, q in enumerate(robots):
            tr = bat.resident_read_trace(b)
            finite = bool(np.all(np.isfinite(tr)))
            mx, rms = tracking_errors(tr, px, py) if finite else (float("nan"), float("nan"))
            q[name] = {"finite": finite, "closest_m": float(np.min(np.hypot(tr[:, 0] - discs[b][0, 0], tr[:, 1] - discs[b][0, 1]))),
                       "rms_m": rms, "max_m": mx}
        bat.close()
    return {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "path": "sinusoid", "radius_m": radius,
            "weight": weight, "robots": robots}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=256, help="timed launches per round (>= 256)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_obstacles_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {"device": props.name, "cus": props.multi_processor_count, "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f n8 %7.2f n32 %7.2f (off spread %.2f)  launch sequence us: off %7.2f n8 %7.2f n32 %7.2f" % (
            p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["n8_kernel_us"], r["n32_kernel_us"], r["spread_off_kernel_us"],
            r["off_iter_us"], r["n8_iter_us"], r["n32_iter_us"]), file=sys.stderr, flush=True)
    stream = torch.cuda.Stream()
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, stream)
    out["resident"] = r
    print("resident B=64 tick us: off %.2f n8 %.2f n32 %.2f (off spread %.2f)" % (r["off_tick_us"], r["n8_tick_us"], r["n32_tick_us"],
                                                                               r["spread_off_tick_us"]), file=sys.stderr, flush=True)
    s = behaviour(args.ticks)
    out["behaviour"] = s
    off = np.array([q["off"]["closest_m"] for q in s["robots"]])
    on = np.array([q["on"]["closest_m"] for q in s["robots"]])
    print("closest approach to the disc centre, m: off median %.3f, on median %.3f, robots farther with the term on: %d / %d" % (
        float(np.median(off)), float(np.median(on)), int(np.sum(on > off)), len(on)), file=sys.stderr)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Shifted weights on batch handles (ccv_mppi_batch_set_min_shift) against the same handle with the mode off, same process,
same inputs: `python tools/batch_shift_bench.py [--out FILE]` (default profiles/batch_shift_bench.json).

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters (B copies of the configuration: the
VARIED kernels are the yardstick, the mode runs on top of them) on the inputs of tools/batch_params_bench.py; shift off and
shift on alternate on that handle round by round (--rounds), each round the mean of --iters (>= 256) event-timed launches
(ccv_mppi_batch_timing_*): off_kernel_us / on_kernel_us the rollout kernel, off_iter_us / on_iter_us the whole launch sequence
(rollout + update), medians over the rounds, and spread_* = max - min of the shift-off rounds.  Diff drive K = 1 000, H = 15,
B = 64 also runs the resident closed loop the same way (device events over --ticks ticks, us per tick).
The sweep leg: the lambda = 0.1 column of tools/batch_params_bench.py's 8 x 8 (lambda, sigma) grid -- eight robots, sigma in
linspace(0.1, 1.0, 8), 256 resident ticks on the sinusoid path -- with shift off and with shift on: RMS / max distance to the
path.  One JSON document goes to stdout (and --out)."""
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

MODES = (("off", False), ("on", True))


def times_us(h, ins, n, it0):
    h.timing_enable(True)
    for i in range(n):
        h.iterate_enqueue(*ins, it0 + i)
    roll, tot, cnt = h.timing_read()
    h.timing_enable(False)
    return roll / cnt, tot / cnt


def summary(res, times, unit):
    for k, v in times.items():
        res[k + unit] = float(np.median(v))
    for k, v in times.items():
        if k.startswith("off"):
            res["spread_" + k + unit] = float(max(v) - min(v))


def measure(p, B, iters, rounds, warmup):
    ins = inputs(p, B)
    h = amd.BatchController([p] * B, B)
    for _name, on in MODES:
        h.set_min_shift(on)
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {"off_kernel": [], "on_kernel": [], "off_iter": [], "on_iter": []}
    kernel = {}
    for r in range(rounds):
        for name, on in MODES:
            h.set_min_shift(on)
            k, t = times_us(h, ins, iters, r * iters)
            times[name + "_kernel"].append(k)
            times[name + "_iter"].append(t)
            kernel[name] = h.last_kernel()
    h.close()
    res = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "kernel": kernel, "rounds": rounds,
           "iters_per_round": iters, "per_round": {k + "_us": v for k, v in times.items()}}
    summary(res, times, "_us")
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    import torch
    kinds = [amd.make_path("sinusoid", length=40.0), amd.make_path("dkan")]
    paths = [kinds[b % 2] for b in range(B)]
    s0 = np.zeros((B, p.nstate))
    for b in range(B):
        px, py = paths[b]
        i = (13 * b) % (len(px) // 4)
        s0[b, 0], s0[b, 1] = px[i], py[i] + 0.02 * ((b % 5) - 2)
        s0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)
    h = amd.BatchController([p] * B, B)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    times = {"off_tick": [], "on_tick": []}
    kernel = {}
    for _r in range(rounds):
        for name, on in MODES:
            h.set_min_shift(on)
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


def sweep_column(ticks, lam=0.1):
    p = configs.diff_drive_defaults(1000, 15)
    sigmas = [float(x) for x in np.linspace(0.1, 1.0, 8)]
    seq = [p.with_(lam=lam, control_noise=s) for s in sigmas]
    B = len(seq)
    px, py = amd.make_path("sinusoid", length=40.0)
    s0 = np.zeros((B, 3))
    s0[:, 0], s0[:, 1], s0[:, 2] = px[0], py[0], np.arctan2(py[1] - py[0], px[1] - px[0])
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)   # (the keys of the grid's first eight robots)
    points = [{"lambda": lam, "sigma": s} for s in sigmas]
    for name, on in MODES:
        bat = amd.BatchController(seq, B, min_shift=on)
        bat.resident_set_paths((px, py))
        bat.resident_set_poses(s0, seeds)
        for i in range(ticks):
            bat.resident_step_enqueue(p.dt, i, advance=i > 0)
        bat.synchronize()
        for b, q in enumerate(points):
            tr = bat.resident_read_trace(b)
            finite = bool(np.all(np.isfinite(tr)))
            mx, rms = tracking_errors(tr, px, py) if finite else (float("nan"), float("nan"))
            q[name] = {"finite": finite, "max_m": mx, "rms_m": rms,
                       "travelled_m": float(np.hypot(*(tr[-1, :2] - tr[0, :2]))) if finite else float("nan")}
        bat.close()
    return {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "path": "sinusoid", "column": points}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=256, help="timed launches per round (>= 256)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_shift_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {"device": props.name, "cus": props.multi_processor_count, "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f on %7.2f (off spread %.2f)  launch sequence us: off %7.2f on %7.2f (off spread %.2f)" % (
            p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["on_kernel_us"], r["spread_off_kernel_us"],
            r["off_iter_us"], r["on_iter_us"], r["spread_off_iter_us"]), file=sys.stderr, flush=True)
    stream = torch.cuda.Stream()
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, stream)
    out["resident"] = r
    print("resident B=64 tick us: off %.2f on %.2f (off spread %.2f)" % (r["off_tick_us"], r["on_tick_us"], r["spread_off_tick_us"]),
          file=sys.stderr, flush=True)
    s = sweep_column(args.ticks)
    out["sweep_lambda_0p1"] = s
    for q in s["column"]:
        print("lambda 0.1 sigma %.3f  rms m: off %.4f on %.4f" % (q["sigma"], q["off"]["rms_m"], q["on"]["rms_m"]), file=sys.stderr)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

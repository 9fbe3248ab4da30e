#!/usr/bin/env python3
"""Shifted weights on batch handles (ccv_mppi_batch_set_min_shift) against the same handle with the mode off, same process,
same inputs: `python tools/batch_shift_bench.py [--out FILE]` (default profiles/batch_shift_bench.json).  The method, the
inputs and both loops are those of tools/bench_support.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters (B copies of the configuration: the
VARIED kernels are the yardstick, the mode runs on top of them); shift off and shift on alternate on that handle round by
round (--rounds), each round the mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): off_kernel_us /
on_kernel_us the rollout kernel, off_iter_us / on_iter_us the whole launch sequence (rollout + update), medians over the
rounds, and spread_* = max - min of the shift-off rounds.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident closed
loop the same way (device events over --ticks ticks, us per tick).
The sweep leg: the lambda = 0.1 column of tools/batch_params_bench.py's 8 x 8 (lambda, sigma) grid -- eight robots, sigma in
linspace(0.1, 1.0, 8), 256 resident ticks on the sinusoid path -- with shift off and with shift on: RMS / max distance to the
path.  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402

MODES = (("off", False), ("on", True))


def set_mode(h, mode):
    h.set_min_shift(mode[1])


def measure(p, B, iters, rounds, warmup):
    h = amd.BatchController([p] * B, B)
    times, kernel = bs.measure_modes(h, bs.inputs(p, B), MODES, set_mode, iters, rounds, warmup)
    h.close()
    res = {**bs.shape(p, B), "kernel": kernel, "rounds": rounds, "iters_per_round": iters}
    bs.summary(res, times, "_us")
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    paths, s0, seeds = bs.fleet(p, B)
    h = bs.resident_handle([p] * B, B, stream, paths)
    times, _wall, kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, MODES, set_mode, ticks, rounds, warmup)
    h.close()
    out = {**bs.shape(p, B), "ticks": ticks, "rounds": rounds, "kernel": kernel}
    bs.summary(out, times, "_tick_us")
    return out


def sweep_column(ticks, lam=0.1):
    p = configs.diff_drive_defaults(1000, 15)
    sigmas = [float(x) for x in np.linspace(0.1, 1.0, 8)]
    seq = [p.with_(lam=lam, control_noise=s) for s in sigmas]
    B = len(seq)
    path = amd.make_path("sinusoid", length=40.0)
    points = [{"lambda": lam, "sigma": s} for s in sigmas]
    for name, on in MODES:
        bat = amd.BatchController(seq, B, min_shift=on)
        # (the seeds are the keys of the grid's first eight robots)
        legs = bs.closed_loop(bat, path, bs.path_start(path, B), bs.fleet_seeds(B), p.dt, ticks,
                              lambda b, tr, finite: {"travelled_m": bs.travelled(tr) if finite else float("nan")})
        bat.close()
        for q, leg in zip(points, legs):
            q[name] = leg
    return {**bs.shape(p, B), "ticks": ticks, "path": "sinusoid", "column": points}


def main():
    args = bs.parser("batch_shift_bench.json", iters=256, ticks=256).parse_args()
    out = {**bs.header(), "configs": []}
    for p, B in bs.varied_plan():
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f on %7.2f (off spread %.2f)  launch sequence us: off %7.2f on %7.2f (off spread %.2f)" % (
            p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["on_kernel_us"], r["spread_off_kernel_us"],
            r["off_iter_us"], r["on_iter_us"], r["spread_off_iter_us"]), file=sys.stderr, flush=True)
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, bs.new_stream())
    out["resident"] = r
    print("resident B=64 tick us: off %.2f on %.2f (off spread %.2f)" % (r["off_tick_us"], r["on_tick_us"], r["spread_off_tick_us"]),
          file=sys.stderr, flush=True)
    s = sweep_column(args.ticks)
    out["sweep_lambda_0p1"] = s
    for q in s["column"]:
        print("lambda 0.1 sigma %.3f  rms m: off %.4f on %.4f" % (q["sigma"], q["off"]["rms_m"], q["on"]["rms_m"]), file=sys.stderr)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

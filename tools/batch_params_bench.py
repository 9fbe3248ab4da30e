#!/usr/bin/env python3
"""Per-instance parameters on batch handles against the shared batch, same process, same inputs:
`python tools/batch_params_bench.py [--out FILE]` (default profiles/batch_params_bench.json).

For every configuration (model, K, H, B), three batch handles on the inputs and by the method of tools/bench_support.py:
  (a) shared_kernel_us   the shared batch (one configuration, today's kernels)
  (b) copies_kernel_us   the batch with per-instance parameters, B copies of the same configuration (the VARIED kernels)
  (c) sweep_kernel_us    the batch with per-instance parameters, a real sweep of sigma, lambda, v_ref, bounds and weights
each the rollout kernel by hipEvents on the dispatch (ccv_mppi_batch_timing_*), mean of --iters (>= 256) launches; the three
alternate round by round (--rounds) and the median is reported.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident
closed loop of the three (device events over --ticks ticks, us per tick).
The sweep leg: diff drive, an 8 x 8 grid of (lambda, sigma) as ONE resident batch of 64 robots on the sinusoid path, 256
ticks from the path's start; every grid point's max / RMS distance to the path over its trace (the metric of
tests/closed_loop_eval.py, calc_e_rmse.py:30-49).  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402


def sweep(p, B):
    """B parameter sets around p: sigma, lambda, v_ref, bounds and weights all vary (bounds inside the fast sin / cos range)"""
    return [p.with_(control_noise=p.control_noise * (0.5 + 0.1 * (b % 11)), lam=p.lam * (0.25 + 0.25 * (b % 7)),
                    v_ref=p.v_ref * (0.6 + 0.05 * (b % 9)), u_min=tuple(x * (0.8 + 0.05 * (b % 5)) for x in p.u_min),
                    u_max=tuple(x * (0.8 + 0.05 * (b % 4)) for x in p.u_max), path_weight=p.path_weight * (0.5 + 0.25 * (b % 6)),
                    v_weight=p.v_weight * (0.5 + 0.2 * (b % 5)), zmp_weight=p.zmp_weight * (0.5 + 0.1 * (b % 3)),
                    roll_v_weight=p.roll_v_weight * (0.5 + 0.1 * (b % 4)), back_weight=p.back_weight * (1.0 + 0.5 * (b % 3)),
                    yaw_weight=p.yaw_weight * (0.5 + 0.1 * (b % 5))) for b in range(B)]


def handles(p, B):
    shared, copies, swept = amd.BatchController(p, B), amd.BatchController(p, B), amd.BatchController(p, B)
    copies.set_params([p] * B)
    swept.set_params(sweep(p, B))
    return {"shared": shared, "copies": copies, "sweep": swept}


def measure(p, B, iters, rounds, warmup):
    """bench_support.measure_modes with three handles in the place of one handle's modes, and the kernel figure alone"""
    ins = bs.inputs(p, B)
    hs = handles(p, B)
    for h in hs.values():
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {k: [] for k in hs}
    for r in range(rounds):
        for k, h in hs.items():
            times[k].append(bs.launch_us(h, lambda i: h.iterate_enqueue(*ins, r * iters + i), iters)[0])
    res = {**bs.shape(p, B), "kernel": {k: h.last_kernel() for k, h in hs.items()}, "rounds": rounds, "iters_per_round": iters}
    bs.summary(res, times, "_kernel_us", baseline=None)
    for h in hs.values():
        h.close()
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    """bench_support.resident_modes, again with the three handles in the place of the modes"""
    paths, s0, seeds = bs.fleet(p, B)
    hs = handles(p, B)
    for h in hs.values():
        h.set_stream(stream.cuda_stream)
        h.resident_set_paths(paths)
    times = {k: [] for k in hs}
    for _r in range(rounds):
        for k, h in hs.items():
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            times[k].append(bs.tick_us(stream, ticks, lambda i: h.resident_step_enqueue(p.dt, warmup + i)))
    out = {**bs.shape(p, B), "ticks": ticks, "rounds": rounds, "kernel": {k: h.last_kernel() for k, h in hs.items()}}
    bs.summary(out, times, "_tick_us", baseline=None)
    for h in hs.values():
        h.close()
    return out


def sweep_leg(ticks):
    p = configs.diff_drive_defaults(1000, 15)
    lams = [float(x) for x in np.geomspace(0.1, 10.0, 8)]
    sigmas = [float(x) for x in np.linspace(0.1, 1.0, 8)]
    grid = [(lam, s) for lam in lams for s in sigmas]
    B = len(grid)
    path = amd.make_path("sinusoid", length=40.0)
    bat = amd.BatchController([p.with_(lam=lam, control_noise=s) for lam, s in grid], B)
    legs, us = bs.closed_loop(bat, path, bs.path_start(path, B), bs.fleet_seeds(B), p.dt, ticks,
                              lambda b, tr, _finite: {"travelled_m": bs.travelled(tr)}, timed=True)
    points = [{"lambda": lam, "sigma": s, "max_m": q["max_m"], "rms_m": q["rms_m"], "travelled_m": q["travelled_m"]}
              for (lam, s), q in zip(grid, legs)]
    kernel = bat.last_kernel()
    bat.close()
    best = min(points, key=lambda q: q["rms_m"])
    return {**bs.shape(p, B), "ticks": ticks, "path": "sinusoid", "kernel": kernel, "wall_us_per_tick": us, "best": best,
            "grid": points}


def main():
    args = bs.parser("batch_params_bench.json", iters=256, ticks=256).parse_args()
    out = {**bs.header(), "configs": []}
    for p, B in bs.varied_plan():
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: shared %7.2f  copies %7.2f  sweep %7.2f" % (
            p.model, p.num_samples, p.horizon, B, r["shared_kernel_us"], r["copies_kernel_us"], r["sweep_kernel_us"]),
            file=sys.stderr, flush=True)
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, bs.new_stream())
    out["resident"] = r
    print("resident B=64 tick us: shared %.2f  copies %.2f  sweep %.2f" % (r["shared_tick_us"], r["copies_tick_us"],
                                                                           r["sweep_tick_us"]), file=sys.stderr, flush=True)
    s = sweep_leg(args.ticks)
    out["sweep"] = s
    print("sweep 8 x 8 (lambda, sigma), %d ticks: best lambda %.3g sigma %.3g rms %.4f m max %.4f m" % (
        s["ticks"], s["best"]["lambda"], s["best"]["sigma"], s["best"]["rms_m"], s["best"]["max_m"]), file=sys.stderr)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per-instance parameters on batch handles against the shared batch, same process, same inputs:
`python tools/batch_params_bench.py [--out FILE]` (default profiles/batch_params_bench.json).

For every configuration (model, K, H, B), three batch handles on the inputs of tools/batch_bench.py:
  (a) shared_kernel_us   the shared batch (one configuration, today's kernels)
  (b) copies_kernel_us   the batch with per-instance parameters, B copies of the same configuration (the VARIED kernels)
  (c) sweep_kernel_us    the batch with per-instance parameters, a real sweep of sigma, lambda, v_ref, bounds and weights
each the rollout kernel by hipEvents on the dispatch (ccv_mppi_batch_timing_*), mean of --iters (>= 256) launches; the three
alternate round by round (--rounds) and the median is reported.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident
closed loop of the three (device events over --ticks ticks, us per tick).
The sweep leg: diff drive, an 8 x 8 grid of (lambda, sigma) as ONE resident batch of 64 robots on the sinusoid path, 256
ticks from the path's start; every grid point's max / RMS distance to the path over its trace (the metric of
tests/closed_loop_eval.py, calc_e_rmse.py:30-49).  One JSON document goes to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402

PATH_OF = {"diff_drive": "sinusoid", "steering_diff_drive": "sinusoid", "full_body": "dkan"}


def inputs(p, B):
    px, py = amd.make_path(PATH_OF[p.model])
    x0, xr, yr = np.zeros((B, p.nstate)), np.zeros((B, p.horizon)), np.zeros((B, p.horizon))
    dt, yaw0 = np.zeros(B), np.zeros(B)
    for b in range(B):
        i = (13 * b) % (len(px) // 2)
        x0[b, 0], x0[b, 1] = px[i], py[i] + 0.02 * ((b % 5) - 2)
        x0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
        dt[b] = p.dt * (1.0 + 0.02 * (b % 3))
        _, xr[b], yr[b], yaw = amd.calc_ref_path(px, py, x0[b, 0], x0[b, 1], p.v_ref, dt[b], p.resolution, p.horizon)
        yaw0[b] = yaw[0]
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)
    return x0, dt, xr, yr, yaw0, seeds


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


def kernel_us(h, ins, n, it0):
    h.timing_enable(True)
    for i in range(n):
        h.iterate_enqueue(*ins, it0 + i)
    roll, _tot, cnt = h.timing_read()
    h.timing_enable(False)
    return roll / cnt


def measure(p, B, iters, rounds, warmup):
    ins = inputs(p, B)
    hs = handles(p, B)
    for h in hs.values():
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {k: [] for k in hs}
    for r in range(rounds):
        for k, h in hs.items():
            times[k].append(kernel_us(h, ins, iters, r * iters))
    res = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B,
           "kernel": {k: h.last_kernel() for k, h in hs.items()}, "rounds": rounds, "iters_per_round": iters,
           "per_round": {k + "_kernel_us": v for k, v in times.items()}}
    for k, v in times.items():
        res[k + "_kernel_us"] = float(np.median(v))
    for h in hs.values():
        h.close()
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
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for i in range(ticks):
                h.resident_step_enqueue(p.dt, warmup + i)
            stop.record(stream)
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) * 1e3 / ticks)
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "rounds": rounds,
           "kernel": {k: h.last_kernel() for k, h in hs.items()}, "per_round": {k + "_tick_us": v for k, v in times.items()}}
    for k, v in times.items():
        out[k + "_tick_us"] = float(np.median(v))
    for h in hs.values():
        h.close()
    return out


def tracking_errors(traj, px, py):
    """tests/closed_loop_eval.py (calc_e_rmse.py:30-49): max and RMS distance of the poses to the path"""
    d = np.sqrt((traj[:, 0:1] - px[None, :]) ** 2 + (traj[:, 1:2] - py[None, :]) ** 2).min(axis=1)
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def sweep_leg(ticks):
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    lams = [float(x) for x in np.geomspace(0.1, 10.0, 8)]
    sigmas = [float(x) for x in np.linspace(0.1, 1.0, 8)]
    grid = [(lam, s) for lam in lams for s in sigmas]
    seq = [p.with_(lam=lam, control_noise=s) for lam, s in grid]
    B = len(seq)
    px, py = amd.make_path("sinusoid", length=40.0)
    bat = amd.BatchController(seq, B)
    bat.resident_set_paths((px, py))
    s0 = np.zeros((B, 3))
    s0[:, 0], s0[:, 1], s0[:, 2] = px[0], py[0], np.arctan2(py[1] - py[0], px[1] - px[0])
    bat.resident_set_poses(s0, np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(ticks):
        bat.resident_step_enqueue(p.dt, i, advance=i > 0)
    bat.synchronize()
    stop.record()
    stop.synchronize()
    points = []
    for b, (lam, s) in enumerate(grid):
        tr = bat.resident_read_trace(b)
        mx, rms = tracking_errors(tr, px, py)
        points.append({"lambda": lam, "sigma": s, "max_m": mx, "rms_m": rms,
                       "travelled_m": float(np.hypot(*(tr[-1, :2] - tr[0, :2])))})
    kernel = bat.last_kernel()
    bat.close()
    best = min(points, key=lambda q: q["rms_m"])
    return {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "ticks": ticks, "path": "sinusoid",
            "kernel": kernel, "wall_us_per_tick": start.elapsed_time(stop) * 1e3 / ticks, "best": best, "grid": points}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=256, help="timed launches per round (>= 256)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_params_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {"device": props.name, "cus": props.multi_processor_count, "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: shared %7.2f  copies %7.2f  sweep %7.2f" % (
            p.model, p.num_samples, p.horizon, B, r["shared_kernel_us"], r["copies_kernel_us"], r["sweep_kernel_us"]),
            file=sys.stderr, flush=True)
    stream = torch.cuda.Stream()
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, stream)
    out["resident"] = r
    print("resident B=64 tick us: shared %.2f  copies %.2f  sweep %.2f" % (r["shared_tick_us"], r["copies_tick_us"],
                                                                           r["sweep_tick_us"]), file=sys.stderr, flush=True)
    s = sweep_leg(args.ticks)
    out["sweep"] = s
    print("sweep 8 x 8 (lambda, sigma), %d ticks: best lambda %.3g sigma %.3g rms %.4f m max %.4f m" % (
        s["ticks"], s["best"]["lambda"], s["best"]["sigma"], s["best"]["rms_m"], s["best"]["max_m"]), file=sys.stderr)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

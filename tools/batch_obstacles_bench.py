#!/usr/bin/env python3
"""The disc-obstacle term of batch handles (ccv_mppi_batch_set_obstacles) against the same handle with the term off, same
process, same inputs: `python tools/batch_obstacles_bench.py [--out FILE]` (default profiles/batch_obstacles_bench.json).  The
method, the inputs and both loops are those of tools/bench_support.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters (B copies of the configuration: the
obstacle-off VARIED kernel is the yardstick); the term off, on with n = 8 and on
with n = 32 discs per instance (weight 1, scattered within 3 m of the window) alternate on that handle round by round
(--rounds), each round the mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the rollout
kernel, *_iter_us the whole launch sequence, medians over the rounds, and spread_* = max - min of the off rounds.  Diff drive
K = 1 000, H = 15, B = 64 also runs the resident closed loop the same way (device events over --ticks ticks, us per tick).
The behavioural leg: 64 robots on the sinusoid path, shifted weights on, each with one disc (r = 0.4 m, weight 200) centred on
a path point ahead; per robot the smallest distance of its trace to the disc's centre with the term off and on, and the RMS
distance to the path.  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402

MODES = (("off", 0), ("n8", 8), ("n32", 32))


def mode_setter(centres):
    discs = {n: bs.scatter(centres, n) for _, n in MODES if n}
    return lambda h, mode: h.set_obstacles(discs[mode[1]] if mode[1] else None, 1.0)


def measure(p, B, iters, rounds, warmup):
    ins = bs.inputs(p, B)
    h = amd.BatchController([p] * B, B)
    times, kernel = bs.measure_modes(h, ins, MODES, mode_setter(bs.window_centres(p, ins)), iters, rounds, warmup)
    h.close()
    res = {**bs.shape(p, B), "kernel": kernel, "rounds": rounds, "iters_per_round": iters}
    bs.summary(res, times, "_us")
    return res


def resident_tick(p, B, ticks, rounds, warmup, stream):
    paths, s0, seeds = bs.fleet(p, B)
    h = bs.resident_handle([p] * B, B, stream, paths)
    times, _wall, kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, MODES, mode_setter(s0[:, :2]), ticks, rounds, warmup)
    h.close()
    out = {**bs.shape(p, B), "ticks": ticks, "rounds": rounds, "kernel": kernel}
    bs.summary(out, times, "_tick_us")
    return out


def behaviour(ticks, B=64, radius=0.4, weight=200.0):
    p = configs.diff_drive_defaults(1000, 15)
    px, py = path = amd.make_path("sinusoid", length=40.0)
    s0 = np.zeros((B, 3))
    discs = []
    for b in range(B):
        i = (5 * b) % (len(px) // 4)
        s0[b] = (px[i], py[i], np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]))
        j = i + 40 + (b % 7)
        discs.append(np.array([[px[j], py[j], radius]]))
    robots = [{"disc": [float(v) for v in discs[b][0]]} for b in range(B)]
    for name, on in (("off", False), ("on", True)):
        bat = amd.BatchController(p, B, min_shift=True)
        if on:
            bat.set_obstacles(discs, weight)
        legs = bs.closed_loop(bat, path, s0, bs.fleet_seeds(B), p.dt, ticks, lambda b, tr, _finite: {
            "closest_m": float(np.min(np.hypot(tr[:, 0] - discs[b][0, 0], tr[:, 1] - discs[b][0, 1])))})
        bat.close()
        for q, leg in zip(robots, legs):
            q[name] = leg
    return {**bs.shape(p, B), "ticks": ticks, "path": "sinusoid", "radius_m": radius, "weight": weight, "robots": robots}


def main():
    args = bs.parser("batch_obstacles_bench.json", iters=256, ticks=256).parse_args()
    out = {**bs.header(), "configs": []}
    for p, B in bs.varied_plan():
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: off %7.2f n8 %7.2f n32 %7.2f (off spread %.2f)  launch sequence us: off %7.2f n8 %7.2f n32 %7.2f" % (
            p.model, p.num_samples, p.horizon, B, r["off_kernel_us"], r["n8_kernel_us"], r["n32_kernel_us"], r["spread_off_kernel_us"],
            r["off_iter_us"], r["n8_iter_us"], r["n32_iter_us"]), file=sys.stderr, flush=True)
    r = resident_tick(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, bs.new_stream())
    out["resident"] = r
    print("resident B=64 tick us: off %.2f n8 %.2f n32 %.2f (off spread %.2f)" % (r["off_tick_us"], r["n8_tick_us"], r["n32_tick_us"],
                                                                               r["spread_off_tick_us"]), file=sys.stderr, flush=True)
    s = behaviour(args.ticks)
    out["behaviour"] = s
    off = np.array([q["off"]["closest_m"] for q in s["robots"]])
    on = np.array([q["on"]["closest_m"] for q in s["robots"]])
    print("closest approach to the disc centre, m: off median %.3f, on median %.3f, robots farther with the term on: %d / %d" % (
        float(np.median(off)), float(np.median(on)), int(np.sum(on > off)), len(on)), file=sys.stderr)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

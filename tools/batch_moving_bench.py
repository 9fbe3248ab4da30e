#!/usr/bin/env python3
"""The moving-disc form of the batch handles' obstacle term (ccv_mppi_batch_set_obstacle_velocities) against the static form on
the same handle, same process, same inputs: `python tools/batch_moving_bench.py [--out FILE]` (default
profiles/batch_moving_bench.json).  The method, the inputs and both loops are those of tools/bench_support.py.

For every configuration (model, K, H, B) ONE batch handle with per-instance parameters and n = 8 and n = 32 discs per
instance (weight 1, scattered within 3 m of the window); per n the
static OBST kernels (no velocity table) and the MOVING kernels (velocities of up to 1.5 m/s) alternate on that handle round by
round (--rounds), each round the mean of --iters (>= 256) event-timed launches (ccv_mppi_batch_timing_*): *_kernel_us the
rollout kernel, *_iter_us the whole launch sequence, medians over the rounds, and spread_static_* = max - min of the static
rounds.  The yardstick is the static kernel of the same run.  Diff drive K = 1 000, H = 15, B = 64 also runs the resident closed
loop with the fleet term (tools/batch_fleet_bench.py's fleet: max_neighbours = 4 and 16 under a range that holds every robot),
prediction off against on, alternating round by round (device events over --ticks ticks, us per tick, spread of the off
rounds).  One JSON document goes to stdout (and --out)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

NS = (8, 32)
MODES = [("static_n%d" % n, n, False) for n in NS] + [("moving_n%d" % n, n, True) for n in NS]
MODES.sort(key=lambda m: m[1])   # static n8, moving n8, static n32, moving n32


def check_moving(mode, kernel):
    assert bool(kernel & capi.BATCH_KERNEL_MOVING) == mode[2]


def measure(p, B, iters, rounds, warmup):
    ins = bs.inputs(p, B)
    discs = {n: bs.scatter(bs.window_centres(p, ins), n) for n in NS}
    vels = {n: bs.velocities(B, n) for n in NS}
    h = amd.BatchController([p] * B, B)
    times, kernel = bs.measure_modes(h, ins, MODES, lambda h, m: h.set_obstacles(discs[m[1]], 1.0, velocities=vels[m[1]] if m[2] else None),
                                     iters, rounds, warmup, check=check_moving)
    h.close()
    res = {**bs.shape(p, B), "kernel": kernel, "rounds": rounds, "iters_per_round": iters}
    bs.summary(res, times, "_us", baseline="static")
    return res


def resident_prediction(p, B, ticks, rounds, warmup, stream, neighbours=(4, 16), radius=0.3, reach=1.0e3):
    paths, s0, seeds = bs.fleet(p, B)
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)
    modes = [(("pred%d" if on else "off%d") % m, m, on) for m in neighbours for on in (False, True)]

    def set_mode(h, mode):
        h.resident_set_fleet(radius, reach, mode[1], 1.0)
        h.resident_set_fleet_prediction(mode[2])

    times, _wall, kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, modes, set_mode, ticks, rounds, warmup, check=check_moving)
    h.close()
    out = {**bs.shape(p, B), "ticks": ticks, "rounds": rounds, "kernel": kernel}
    bs.summary(out, times, "_tick_us")
    return out


def main():
    args = bs.parser("batch_moving_bench.json", iters=256, ticks=256).parse_args()
    out = {**bs.header(), "configs": []}
    for p, B in bs.varied_plan():
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-12s K=%6d H=%3d B=%4d  kernel us: n8 static %7.2f moving %7.2f (static spread %.2f)  n32 static %7.2f moving %7.2f "
              "(static spread %.2f)" % (p.model, p.num_samples, p.horizon, B, r["static_n8_kernel_us"], r["moving_n8_kernel_us"],
                                        r["spread_static_n8_kernel_us"], r["static_n32_kernel_us"], r["moving_n32_kernel_us"],
                                        r["spread_static_n32_kernel_us"]), file=sys.stderr, flush=True)
    r = resident_prediction(configs.diff_drive_defaults(1000, 15), 64, args.ticks, args.rounds, args.warmup, bs.new_stream())
    out["resident_fleet"] = r
    print("resident fleet B=64 tick us: " + "  ".join("%s %.2f" % (k[:-3], v) for k, v in r.items() if k.endswith("_tick_us")),
          file=sys.stderr, flush=True)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

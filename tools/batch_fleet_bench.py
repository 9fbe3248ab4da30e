#!/usr/bin/env python3
"""The fleet term of batch handles (ccv_mppi_batch_resident_set_fleet) against the same handle with the term off, same process,
same poses: `python tools/batch_fleet_bench.py [--out FILE]` (default profiles/batch_fleet_bench.json).  The method, the fleet
and the resident loop are those of tools/bench_support.py.

The resident tick (device events over --ticks ticks, us per tick) of ONE handle per configuration: diff drive K = 1 000, H = 15
at B = 8, 64, 256 and full body K = 10 000, H = 15 at B = 4.  For max_neighbours m in {4, 16} two modes alternate round by
round (--rounds): "off" = the term off with m static discs per robot, scattered within 3 m of its start, so that the same
rollout kernel does the same loop work, and "on" = the term on with max_neighbours = m and a range that holds every robot.
Medians over the rounds, and spread_* = max - min of the off rounds: the yardstick is the off mode of the same run.
`--trace` runs one short on-mode loop per configuration and nothing else, for a kernel-trace run of its own
(rocprofv3 --kernel-trace --stats -- python tools/batch_fleet_bench.py --trace): the k_finalize_advance_batch* time is read
from its statistics.  One JSON document goes to stdout (and --out)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
from ccv_mppi_path_tracker_amd import configs  # noqa: E402

NEIGHBOURS = (4, 16)
RADIUS, WEIGHT, RANGE = 0.3, 1.0, 1.0e3


def resident_tick(p, B, ticks, rounds, warmup, stream, trace=False):
    paths, s0, seeds = bs.fleet(p, B)
    discs = {m: bs.scatter(s0[:, :2], m) for m in NEIGHBOURS}
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)
    modes = [("on%d" % m, True, m) for m in NEIGHBOURS] if trace else \
            [(("on%d" if on else "off%d") % m, on, m) for m in NEIGHBOURS for on in (False, True)]

    def set_mode(h, mode):
        _name, on, m = mode
        if on:
            h.set_obstacles(None)
            h.resident_set_fleet(RADIUS, RANGE, m, WEIGHT)
        else:
            h.resident_set_fleet(None)
            h.set_obstacles(discs[m], WEIGHT)

    times, _wall, kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, modes, set_mode, ticks, 1 if trace else rounds, warmup)
    h.close()
    out = {**bs.shape(p, B), "ticks": ticks, "rounds": rounds, "kernel": kernel}
    bs.summary(out, times, "_tick_us")
    return out


def main():
    ap = bs.parser("batch_fleet_bench.json", ticks=256)
    ap.add_argument("--trace", action="store_true", help="one short on-mode loop per configuration, for a kernel-trace run")
    args = ap.parse_args()
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (8, 64, 256)] + [(configs.full_body_defaults(10000, 15), 4)]
    out = {**bs.header(), "radius_m": RADIUS, "range_m": RANGE, "resident": []}
    stream = bs.new_stream()
    for p, B in plan:
        r = resident_tick(p, B, 64 if args.trace else args.ticks, args.rounds, args.warmup, stream, args.trace)
        out["resident"].append(r)
        print("%-12s K=%6d B=%4d tick us: %s" % (p.model, p.num_samples, B, "  ".join(
            "%s %.2f" % (k[:-3], v) for k, v in r.items() if k.endswith("_tick_us"))), file=sys.stderr, flush=True)
    if not args.trace:
        bs.emit(out, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Best candidates and optimal paths of every instance of a batch (ccv_mppi_batch_read_best_candidates, _read_optimal_paths;
DESIGN.md section 10l) against what a caller of the parent commit has to do: `python tools/batch_feed_bench.py [--out FILE]`
(default profiles/batch_feed_bench.json).  Diff drive K = 1 000, H = 15; B in {1, 64, 1024}; N in {1, 10, 100}.

Per (B, N), in one process, the two routes in alternating repetitions, medians of --rounds beside the rounds themselves
(wall time of the calls, us):
  `best_us`         one read_best_candidates(N) with paths;  `best_nopaths_us`  the same without the states
  `parent_best_us`  per instance one read_costs, a numpy argsort (stable: the same order) and one read_candidates per index
Per B:
  `paths_us`         one read_optimal_paths
  `parent_paths_us`  get_nominal, then H - 1 ccv_mppi_plant_step calls per instance on the host
  `tick_us` / `tick_best_us`  the period of the resident loop over --ticks ticks (device events around the loop, us per tick)
                     without and with one read_best_candidates(10, no paths) after every tick -- the call synchronises, so the
                     second figure is the period of a loop that publishes every tick
`single_large`: one instance of K = 65 536 (one workgroup selects among all of them: the design point is many small instances),
N = 100, after a host-record tick: `best_us`, `best_nopaths_us`, and `read_costs_us`, one read_costs of all K for scale.
Every figure is recorded; none is asserted.  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402

BATCHES = (1, 64, 1024)
COUNTS = (1, 10, 100)


def parent_best(h, n):
    """the parent commit's route to the same arrays"""
    idx, cost, xy = np.empty((h.B, n), dtype=np.int32), np.empty((h.B, n)), np.empty((h.B, n, h.H, 2))
    for b in range(h.B):
        c = h.read_costs(b)
        idx[b] = np.argsort(c, kind="stable")[:n]
        cost[b] = c[idx[b]]
        for j in range(n):
            xy[b, j] = h.read_candidates(b, first=int(idx[b, j]), count=1)[0]
    return idx, cost, xy


def parent_paths(h, p, poses, dt):
    u = h.get_nominal()
    out = np.empty((h.B, h.H - 1, 3))
    for b in range(h.B):
        s = poses[b].copy()
        for i in range(h.H - 1):
            out[b, i] = s[:3]
            s = amd.plant_step(p.model, s, u[b, i], dt)
    return out


def one_batch(p, B, rounds, ticks, warmup):
    paths, s0, seeds = bs.fleet(p, B)
    stream = bs.new_stream()
    h = amd.BatchController(p, B)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    h.resident_set_poses(s0, seeds)
    for i in range(warmup):
        h.resident_step_enqueue(p.dt, i, advance=i > 0)
    h.synchronize()
    out = {"B": B, "counts": []}
    for n in COUNTS:
        new, lean, old = [], [], []
        for _ in range(rounds):
            t, got = bs.wall_us(lambda: h.read_best_candidates(n))
            new.append(t)
            lean.append(bs.wall_us(lambda: h.read_best_candidates(n, with_paths=False))[0])
            t, want = bs.wall_us(lambda: parent_best(h, n))
            old.append(t)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        out["counts"].append({"N": n, "best_us": bs.stats(new), "best_nopaths_us": bs.stats(lean), "parent_best_us": bs.stats(old)})
        print("B=%4d N=%3d: best %.1f us (no paths %.1f), parent's route %.1f us" % (B, n, np.median(new), np.median(lean), np.median(old)),
              file=sys.stderr, flush=True)
    poses = h.resident_read()[0]
    new, old = [], []
    for _ in range(rounds):
        t, got = bs.wall_us(h.read_optimal_paths)
        new.append(t)
        t, want = bs.wall_us(lambda: parent_paths(h, p, poses, p.dt))
        old.append(t)
        assert got.tobytes() == want.tobytes()
    out["paths_us"], out["parent_paths_us"] = bs.stats(new), bs.stats(old)
    period = {False: [], True: []}
    for _ in range(rounds):
        for feed in (False, True):
            h.resident_set_poses(s0, seeds)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            h.synchronize()

            def tick(i):
                h.resident_step_enqueue(p.dt, warmup + i)
                if feed:
                    h.read_best_candidates(10, with_paths=False)

            period[feed].append(bs.tick_us(stream, ticks, tick))
    out["tick_us"], out["tick_best_us"] = bs.stats(period[False]), bs.stats(period[True])
    print("B=%4d: optimal paths %.1f us, parent's route %.1f us; resident tick %.2f us, with best candidates every tick %.2f us"
          % (B, np.median(new), np.median(old), np.median(period[False]), np.median(period[True])), file=sys.stderr, flush=True)
    h.close()
    return out


def single_large(rounds):
    p = configs.diff_drive_defaults(65536, 15)
    px, py = amd.make_path("sinusoid")
    x0 = np.array([[px[5], py[5] + 0.02, 0.0]])
    _, xr, yr, yaw = amd.calc_ref_path(px, py, x0[0, 0], x0[0, 1], p.v_ref, p.dt, p.resolution, p.horizon)
    h = amd.BatchController(p, 1)
    h.iterate_enqueue(x0, p.dt, xr[None], yr[None], yaw[0], 7, 0)
    h.synchronize()
    h.read_best_candidates(100)   # (warm-up: the scratch buffer)
    new, lean, costs = [], [], []
    for _ in range(rounds):
        new.append(bs.wall_us(lambda: h.read_best_candidates(100))[0])
        lean.append(bs.wall_us(lambda: h.read_best_candidates(100, with_paths=False))[0])
        costs.append(bs.wall_us(lambda: h.read_costs(0))[0])
    h.close()
    print("B=1 K=65536 N=100: best %.1f us (no paths %.1f), one read_costs of all K %.1f us" % (np.median(new), np.median(lean), np.median(costs)),
          file=sys.stderr, flush=True)
    return {"B": 1, "K": 65536, "N": 100, "best_us": bs.stats(new), "best_nopaths_us": bs.stats(lean), "read_costs_us": bs.stats(costs)}


def main():
    args = bs.parser("batch_feed_bench.json", ticks=256, rounds=5).parse_args()
    p = configs.diff_drive_defaults(1000, 15)
    out = {**bs.header(), "model": p.model, "K": p.num_samples, "H": p.horizon, "rounds": args.rounds, "ticks": args.ticks,
           "batches": [one_batch(p, B, args.rounds, args.ticks, args.warmup) for B in BATCHES], "single_large": single_large(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

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
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402
from batch_obstacles_bench import fleet  # noqa: E402

BATCHES = (1, 64, 1024)
COUNTS = (1, 10, 100)


def stats(v):
    return {"median": float(np.median(v)), "rounds": [float(x) for x in v]}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


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
    import torch
    paths, s0, seeds = fleet(p, B)
    stream = torch.cuda.Stream()
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
            t, got = timed(lambda: h.read_best_candidates(n))
            new.append(t)
            lean.append(timed(lambda: h.read_best_candidates(n, with_paths=False))[0])
            t, want = timed(lambda: parent_best(h, n))
            old.append(t)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        out["counts"].append({"N": n, "best_us": stats(new), "best_nopaths_us": stats(lean), "parent_best_us": stats(old)})
        print("B=%4d N=%3d: best %.1f us (no paths %.1f), parent's route %.1f us" % (B, n, np.median(new), np.median(lean), np.median(old)),
              file=sys.stderr, flush=True)
    poses = h.resident_read()[0]
    new, old = [], []
    for _ in range(rounds):
        t, got = timed(h.read_optimal_paths)
        new.append(t)
        t, want = timed(lambda: parent_paths(h, p, poses, p.dt))
        old.append(t)
        assert got.tobytes() == want.tobytes()
    out["paths_us"], out["parent_paths_us"] = stats(new), stats(old)
    period = {False: [], True: []}
    for _ in range(rounds):
        for feed in (False, True):
            h.resident_set_poses(s0, seeds)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            h.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            for i in range(ticks):
                h.resident_step_enqueue(p.dt, warmup + i)
                if feed:
                    h.read_best_candidates(10, with_paths=False)
            stop.record(stream)
            stop.synchronize()
            period[feed].append(start.elapsed_time(stop) * 1e3 / ticks)
    out["tick_us"], out["tick_best_us"] = stats(period[False]), stats(period[True])
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
        new.append(timed(lambda: h.read_best_candidates(100))[0])
        lean.append(timed(lambda: h.read_best_candidates(100, with_paths=False))[0])
        costs.append(timed(lambda: h.read_costs(0))[0])
    h.close()
    print("B=1 K=65536 N=100: best %.1f us (no paths %.1f), one read_costs of all K %.1f us" % (np.median(new), np.median(lean), np.median(costs)),
          file=sys.stderr, flush=True)
    return {"B": 1, "K": 65536, "N": 100, "best_us": stats(new), "best_nopaths_us": stats(lean), "read_costs_us": stats(costs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_feed_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    p = configs.diff_drive_defaults(1000, 15)
    out = {"device": props.name, "cus": props.multi_processor_count, "model": p.model, "K": p.num_samples, "H": p.horizon,
           "rounds": args.rounds, "ticks": args.ticks, "batches": [one_batch(p, B, args.rounds, args.ticks, args.warmup) for B in BATCHES], "single_large": single_large(args.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

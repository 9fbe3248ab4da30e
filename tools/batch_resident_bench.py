#!/usr/bin/env python3
"""Closed loops of B robots per tick, three ways, same process: `python tools/batch_resident_bench.py [--out FILE]`.

For every configuration (model, K, H, B), each instance on its own path (even b the sinusoid, odd b dkan) and start pose:
  resident_batch_us     (a) the batch handle's device-resident loop: one ccv_mppi_batch_resident_step_enqueue per tick
                        (two launches: the fused update + prologue, and the batched rollout)
  resident_singles_us   (b) B single handles' device-resident loops, stepped one after another on one stream
  host_prologue_us      (c) the batch with the prologue on the host: calc_ref_path + plant_step per instance, then one
                        blocking BatchController.iterate
per tick, from device events on the stream every handle runs on, over --ticks (>= 256) ticks after --warmup ticks from the
start poses; the three alternate round by round (--rounds), the median is reported (the method of tools/bench_support.py,
the three legs in the place of one handle's modes).  host_nonfinite_ticks counts the host
leg's instance-ticks whose command was not finite (the pose is then held: ccv_mppi_plant_step refuses it).  One JSON document
goes to stdout (and --out, by default profiles/batch_resident_bench.json)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402


def measure(p, B, ticks, rounds, warmup, stream):
    paths, s0, seeds = bs.fleet(p, B)
    sp = stream.cuda_stream
    # (a) the batched resident loop
    res = amd.BatchController(p, B)
    res.set_stream(sp)
    res.resident_set_paths(paths)
    res.resident_set_poses(s0, seeds)
    # (b) B single resident handles
    singles = []
    for b in range(B):
        g = amd.MPPIController(p)
        g.set_stream(sp)
        g.resident_set_path(*paths[b])
        g.resident_set_pose(s0[b])
        singles.append(g)
    # (c) the batch with the host prologue
    host = amd.BatchController(p, B)
    host.set_stream(sp)
    state = {"s": s0.copy(), "u": None, "nonfinite": 0}
    it = [0]

    def tick_a(_i):
        res.resident_step_enqueue(p.dt, it[0], advance=it[0] > 0)
        it[0] += 1

    def tick_b(_i):
        for b, g in enumerate(singles):
            g.resident_step_enqueue(p.dt, int(seeds[b]), it[0], advance=it[0] > 0)
        it[0] += 1

    def tick_c(_i):
        s, u = state["s"], state["u"]
        if u is not None:
            ok = np.all(np.isfinite(u[:, 0]), axis=1)
            state["nonfinite"] += int(B - ok.sum())
            s = np.array([amd.plant_step(p.model, s[b], u[b][0], p.dt) if ok[b] else s[b] for b in range(B)])
        xr, yr, yaw0 = np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B)
        for b in range(B):
            _, xr[b], yr[b], yaw = amd.calc_ref_path(paths[b][0], paths[b][1], s[b, 0], s[b, 1], p.v_ref, p.dt,
                                                     p.resolution, p.horizon)
            yaw0[b] = yaw[0]
        state["u"] = host.iterate(s, p.dt, xr, yr, yaw0, seeds, it[0], want_stats=False)
        state["s"] = s
        it[0] += 1

    def reset_a():
        res.resident_set_poses(s0, seeds)

    def reset_b():
        for b, g in enumerate(singles):
            g.resident_set_pose(s0[b])

    def reset_c():
        state["s"], state["u"] = s0.copy(), None

    # every round starts from the start poses (and a warm-up): the robots stay on their paths, where no weight underflows
    legs = {"resident_batch_us": (reset_a, tick_a), "resident_singles_us": (reset_b, tick_b),
            "host_prologue_us": (reset_c, tick_c)}
    per_round = {k: [] for k in legs}
    for _r in range(rounds):
        for k, (reset, tick) in legs.items():
            reset()
            it[0] = 0
            for i in range(warmup):   # (clocks up, code objects loaded, pools settled)
                tick(i)
            stream.synchronize()
            per_round[k].append(bs.tick_us(stream, ticks, tick))
            stream.synchronize()
    out = {**bs.shape(p, B), "kernel": res.last_kernel(), "rounds": rounds,
           "ticks_per_round": ticks, "host_nonfinite_ticks": state["nonfinite"], "per_round": per_round}
    for k, v in per_round.items():
        out[k] = float(np.median(v))
    res.close()
    host.close()
    for g in singles:
        g.close()
    return out


def main():
    args = bs.parser("batch_resident_bench.json", ticks=256).parse_args()
    out = {**bs.header(), "configs": []}
    stream = bs.new_stream()
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 8, 64, 256)] + \
           [(configs.steering_defaults(10000, 15), B) for B in (1, 4, 16)] + \
           [(configs.full_body_defaults(10000, 15), B) for B in (1, 4, 16)]
    for p, B in plan:
        r = measure(p, B, args.ticks, args.rounds, args.warmup, stream)
        out["configs"].append(r)
        print("%-20s K=%6d H=%3d B=%4d  resident batch %8.2f us/tick  %d single resident handles %9.2f  host prologue %9.2f" % (
            p.model, p.num_samples, p.horizon, B, r["resident_batch_us"], B, r["resident_singles_us"], r["host_prologue_us"]),
            file=sys.stderr, flush=True)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

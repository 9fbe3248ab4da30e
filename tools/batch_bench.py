#!/usr/bin/env python3
"""Batch handles against single handles, same process, same inputs: `python tools/batch_bench.py [--out FILE] [--iters N]`.

For every configuration (model, K, H, B): B instances on poses along the model's path with distinct dt and seeds, then
  batch_kernel_us     the batched rollout kernel (hipEvents on the dispatch, ccv_mppi_batch_timing_*), mean of >= 256 launches
  batch_iter_us       its whole launch sequence (record copy, rollout, update) by the same events
  batch_blocking_us   wall time of one blocking ccv_mppi_batch_iterate (mailbox), mean over the timed rounds
  singles_kernel_us   the B single handles' rollout kernels, summed (the same events), and singles_blocking_us: B blocking
                      ccv_mppi_iterate one after another
  rollouts_per_s      B * K / blocking time, batch and singles
  mailbox_blocking_us / copy_blocking_us   the blocking call with the result forced through the pinned mailbox
                      (CCV_MPPI_BATCH_MAIL=1) or through one copy + stream synchronisation (CCV_MPPI_MAILBOX=0): the
                      batch handle takes the mailbox only up to a single handle's largest one
Batch and singles alternate round by round (--rounds): the method of tools/bench_support.py.  The C2-shaped
batch (B = 64 x K = 1 024, H = 50) is compared with the 65 536-sample single handle too (c2_single_kernel_us).  One JSON
document goes to stdout (and --out)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import configs  # noqa: E402


def blocking_with(env, p, B, ins, iters, warmup):
    """mean blocking-call us of a batch handle created under the environment settings `env`"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        bat = amd.BatchController(p, B)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for _ in range(warmup):
        bat.iterate(*ins, 0, want_stats=False)
    t0 = time.perf_counter()
    for i in range(iters):
        bat.iterate(*ins, i, want_stats=False)
    us = (time.perf_counter() - t0) / iters * 1e6
    bat.close()
    return us


def measure(p, B, iters, rounds, warmup):
    x0, dt, xr, yr, yaw0, seeds = bs.inputs(p, B)
    bat = amd.BatchController(p, B)
    singles = [amd.MPPIController(p) for _ in range(B)]
    it = [0]

    def bstep(_i):
        bat.iterate_enqueue(x0, dt, xr, yr, yaw0, seeds, it[0])
        it[0] += 1

    def sstep(g, b):
        return lambda _i: g.iterate_enqueue(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), it[0])

    for _ in range(warmup):   # (clocks up, code objects loaded, pools settled)
        bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
        for b, g in enumerate(singles):
            g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), 0, want_stats=False)
    res = bs.shape(p, B)
    bk, bi, sk, bb, sb = [], [], [], [], []
    for _r in range(rounds):
        k, t = bs.launch_us(bat, bstep, iters)
        bk.append(k)
        bi.append(t)
        tk = 0.0
        n_single = max(8, iters // B)
        for b, g in enumerate(singles):
            tk += bs.launch_us(g, sstep(g, b), n_single)[0]
        sk.append(tk)
        t0 = time.perf_counter()
        for i in range(iters):
            bat.iterate(x0, dt, xr, yr, yaw0, seeds, i, want_stats=False)
        bb.append((time.perf_counter() - t0) / iters * 1e6)
        n_rounds = max(4, iters // B)
        t0 = time.perf_counter()
        for i in range(n_rounds):
            for b, g in enumerate(singles):
                g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), i, want_stats=False)
        sb.append((time.perf_counter() - t0) / n_rounds * 1e6)
    ins = (x0, dt, xr, yr, yaw0, seeds)
    res["mailbox_blocking_us"] = blocking_with({"CCV_MPPI_BATCH_MAIL": "1"}, p, B, ins, iters, warmup)
    res["copy_blocking_us"] = blocking_with({"CCV_MPPI_MAILBOX": "0"}, p, B, ins, iters, warmup)
    med = lambda v: float(np.median(v))
    res.update(batch_kernel_us=med(bk), batch_iter_us=med(bi), batch_blocking_us=med(bb), singles_kernel_us=med(sk),
               singles_blocking_us=med(sb), batch_rollouts_per_s=B * p.num_samples / (med(bb) * 1e-6),
               singles_rollouts_per_s=B * p.num_samples / (med(sb) * 1e-6), single_kernel_us=med(sk) / B,
               single_blocking_us=med(sb) / B, kernel=bat.last_kernel(), rounds=rounds, iters_per_round=iters,
               per_round={"batch_kernel_us": bk, "batch_blocking_us": bb, "singles_kernel_us": sk, "singles_blocking_us": sb})
    bat.close()
    for g in singles:
        g.close()
    return res


def main():
    args = bs.parser(None, iters=256).parse_args()
    plan = [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 8, 64, 256)] + \
           [(configs.steering_defaults(10000, 15), B) for B in (1, 4, 16)] + \
           [(configs.full_body_defaults(10000, 15), B) for B in (1, 4, 16)] + \
           [(configs.workload("C2").params.with_(num_samples=1024), 64)]
    out = {**bs.header(), "configs": []}
    for p, B in plan:
        r = measure(p, B, args.iters, args.rounds, args.warmup)
        out["configs"].append(r)
        print("%-20s K=%6d H=%3d B=%4d  kernel %8.2f us (singles %9.2f)  blocking %8.2f us (singles %9.2f; mailbox %.2f, copy %.2f)" % (
            p.model, p.num_samples, p.horizon, B, r["batch_kernel_us"], r["singles_kernel_us"], r["batch_blocking_us"],
            r["singles_blocking_us"], r["mailbox_blocking_us"], r["copy_blocking_us"]), file=sys.stderr, flush=True)
    # the C2-shaped batch against the 65 536-sample single handle of C2
    p = configs.workload("C2").params
    x0, dt, xr, yr, yaw0, seeds = bs.inputs(p, 1)
    g = amd.MPPIController(p)
    for _ in range(args.warmup):
        g.iterate(x0[0], dt[0], xr[0], yr[0], yaw0[0], 1, 0, want_stats=False)
    ks = [bs.launch_us(g, lambda i: g.iterate_enqueue(x0[0], dt[0], xr[0], yr[0], yaw0[0], 1, i), args.iters)[0]
          for _ in range(args.rounds)]
    out["c2_single_kernel_us"] = float(np.median(ks))
    out["c2_single_kernel_us_per_round"] = ks
    g.close()
    print("C2 single handle K=65536: kernel %.2f us" % out["c2_single_kernel_us"], file=sys.stderr)
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

"""What the tools/batch_*_bench.py tools share, written once: their inputs, their timing primitives, their two loops, their
closed-loop leg, their summaries and the tail of their documents.  No tool imports another tool; every tool imports this module.

The measuring method.  A feature is measured against a baseline in the same process, on ONE handle and the same inputs: the
modes of a tool's mode table alternate round by round (--rounds), so that all of them see the same clock and the same
neighbours, and what is reported is the median over the rounds, beside the rounds themselves and the spread, max - min, of the
baseline mode's rounds -- a difference between two modes below the baseline's spread is not a difference.
  measure_modes    the blocking path: per mode a warm-up of blocking iterate calls, then per round and mode the mean of `iters`
                   (>= 256) enqueued launches by the handle's own events (timing_enable / timing_read): the rollout kernel and
                   the whole launch sequence; iteration numbers r * iters + i.
  resident_modes   the resident closed loop: per round and mode the poses go back to the start, `warmup` ticks run (the first
                   without advancing), then two device events bracket `ticks` calls: us per tick.  The costmap family
                   synchronises after the warm-up, takes the wall clock of the same loop too, and enqueues a mode's map work
                   before or after the step inside the timed region: those are this loop's parameters.
The loops reach torch through event_pair alone, so a CPU test puts a counter in its place."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402

PATH_OF = {"diff_drive": "sinusoid", "steering_diff_drive": "sinusoid", "full_body": "dkan"}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def fleet_seeds(B):
    return np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)


def inputs(p, B):
    """the per-call arrays of the blocking path: B poses along the model's path with distinct dt and seeds"""
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
    return x0, dt, xr, yr, yaw0, fleet_seeds(B)


def fleet(p, B):
    """(paths, start poses, seeds) of a resident fleet: even b on the sinusoid, odd b on dkan (a round's ticks stay on the path)"""
    kinds = [amd.make_path("sinusoid", length=40.0), amd.make_path("dkan")]
    paths = [kinds[b % 2] for b in range(B)]
    s0 = np.zeros((B, p.nstate))
    for b in range(B):
        px, py = paths[b]
        i = (13 * b) % (len(px) // 4)
        s0[b, 0], s0[b, 1] = px[i], py[i] + 0.02 * ((b % 5) - 2)
        s0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
    return paths, s0, fleet_seeds(B)


def path_start(path, B):
    """[B][3]: every robot on the first point of the path, heading along it"""
    px, py = path
    s0 = np.zeros((B, 3))
    s0[:, 0], s0[:, 1], s0[:, 2] = px[0], py[0], np.arctan2(py[1] - py[0], px[1] - px[0])
    return s0


def varied_plan():
    """the (configuration, B) list of the tools that measure a mode of the VARIED kernels on the blocking path"""
    return [(configs.diff_drive_defaults(1000, 15), B) for B in (1, 64, 256)] + \
           [(configs.full_body_defaults(10000, 15), 4), (configs.workload("C2").params.with_(num_samples=1024), 64)]


def window_centres(p, ins):
    """[B][2]: x_ref, y_ref in the middle of the windows of inputs(p, B)"""
    return np.stack([ins[2][:, p.horizon // 2], ins[3][:, p.horizon // 2]], axis=1)


def scatter(centres, n, seed=5):
    """n discs per instance within 3 m of `centres` [B][2], radius 0.2 .. 0.5 m"""
    rng = np.random.default_rng(seed)
    B = len(centres)
    d = np.zeros((B, n, 3))
    d[:, :, :2] = np.asarray(centres)[:, None, :] + rng.uniform(-3.0, 3.0, (B, n, 2))
    d[:, :, 2] = rng.uniform(0.2, 0.5, (B, n))
    return list(d)


def velocities(B, n, seed=6):
    """the velocities of scatter's discs, up to 1.5 m/s an axis"""
    return list(np.random.default_rng(seed).uniform(-1.5, 1.5, (B, n, 2)))


def layer(nx, ny, seed=9):
    """an occupancy layer uint8 [ny][nx], 2 % of the cells occupied"""
    return np.where(np.random.default_rng(seed).random((ny, nx)) < 0.02, 255, 0).astype(np.uint8)


def inflation(R, resolution):
    """the inflation profile of R cells"""
    infl = batch.inflation_profile(R * resolution, resolution)
    assert infl[0] == R
    return infl


def tracking_errors(traj, px, py):
    """tests/closed_loop_eval.py (calc_e_rmse.py:30-49): max and RMS distance of the poses to the path"""
    d = np.sqrt((traj[:, 0:1] - px[None, :]) ** 2 + (traj[:, 1:2] - py[None, :]) ** 2).min(axis=1)
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def travelled(trace):
    return float(np.hypot(*(trace[-1, :2] - trace[0, :2])))


# ---- timing primitives -----------------------------------------------------------------------------------------------------------
def event_pair(stream=None, idle_device=False):
    """-> (start, stop, elapsed_us): start() and stop() record a device event each on `stream`, stop() waits for its event too;
    elapsed_us() is the time between the two.  With idle_device the whole device is synchronised first."""
    import torch
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if idle_device:
        torch.cuda.synchronize()

    def stop():
        last.record(stream)
        last.synchronize()

    return (lambda: first.record(stream)), stop, (lambda: first.elapsed_time(last) * 1e3)


def launch_us(h, step, n):
    """(rollout-kernel us, launch-sequence us), means over n enqueued step(i) by the events of h, a batch or a single handle"""
    h.timing_enable(True)
    for i in range(n):
        step(i)
    roll, tot, cnt = h.timing_read()
    h.timing_enable(False)
    return roll / cnt, tot / cnt


def tick_us(stream, ticks, tick, wall=False):
    """us per tick by device events around `ticks` calls of tick(i) on `stream`; with `wall`, (that, wall us per tick of the loop)"""
    start, stop, elapsed_us = event_pair(stream)
    t0 = time.perf_counter()
    start()
    for i in range(ticks):
        tick(i)
    stop()
    wall_us = (time.perf_counter() - t0) * 1e6 / ticks
    return (elapsed_us() / ticks, wall_us) if wall else elapsed_us() / ticks


def wall_us(fn):
    """(wall us of fn(), what it returned)"""
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def one_call_ms_and_us(h, stream, rounds, call, again=None):
    """per round the wall ms of call() and a synchronisation, then the us between two events on `stream` around again() (by
    default the same call) -> (stats of the ms, stats of the us)"""
    ms, us = [], []
    for _ in range(rounds):
        ms.append(wall_us(lambda: (call(), h.synchronize()))[0] * 1e-3)
        us.append(tick_us(stream, 1, lambda _i: (again or call)()))
    return stats(ms), stats(us)


def idle_call_us(h, call, rounds):
    """stats of the host us of one call(i) with the stream idle and a staging slot free (fewer calls than slots between two
    synchronisations): what the call costs the thread that makes it.  8 * rounds repetitions, the first `rounds` dropped."""
    n, out = capi.OCC_PATCH_SLOTS - 1, []

    def burst():
        for i in range(n):
            call(i)

    for _r in range(8 * rounds):
        h.synchronize()
        out.append(wall_us(burst)[0] / n)
    return stats(out[rounds:])


# ---- the two loops ---------------------------------------------------------------------------------------------------------------
def mode_name(mode):
    """a mode table's rows are names, or tuples that begin with one"""
    return mode if isinstance(mode, str) else mode[0]


def measure_modes(h, ins, modes, set_mode, iters, rounds, warmup, check=None):
    """the blocking path of one handle -> (times {name_kernel, name_iter: us per round}, kernel {name: id}); check(mode, id)"""
    for mode in modes:
        set_mode(h, mode)
        for i in range(warmup):
            h.iterate(*ins, i, want_stats=False)
    times = {mode_name(m) + s: [] for m in modes for s in ("_kernel", "_iter")}
    kernel = {}
    for r in range(rounds):
        for mode in modes:
            name = mode_name(mode)
            set_mode(h, mode)
            k, t = launch_us(h, lambda i: h.iterate_enqueue(*ins, r * iters + i), iters)
            times[name + "_kernel"].append(k)
            times[name + "_iter"].append(t)
            kernel[name] = h.last_kernel()
            if check:
                check(mode, kernel[name])
    return times, kernel


def resident_handle(seq, B, stream, paths, **kw):
    """a batch handle on `stream` with the fleet's paths set"""
    h = amd.BatchController(seq, B, **kw)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    return h


def check_grid(_mode, kernel):
    assert kernel & capi.BATCH_KERNEL_GRID


def resident_modes(h, stream, s0, seeds, dt, modes, set_mode, ticks, rounds, warmup, before_step=None, after_step=None,
                   costmap_form=False, check=None):
    """the resident loop of one handle (stream and paths set) -> (times {name: us per tick per round}, wall, kernel {name: id}).
    before_step(mode, i) / after_step(mode, i) are what a mode enqueues besides the step, inside the timed region;
    costmap_form synchronises after the warm-up and fills `wall` with the wall us per tick of the same loop; check(mode, id)."""
    times, wall, kernel = {mode_name(m): [] for m in modes}, {mode_name(m): [] for m in modes}, {}
    for _r in range(rounds):
        for mode in modes:
            name = mode_name(mode)
            set_mode(h, mode)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):   # (clocks up, code objects loaded, pools settled)
                h.resident_step_enqueue(dt, i, advance=i > 0)
            if costmap_form:
                h.synchronize()

            def tick(i):
                if before_step:
                    before_step(mode, i)
                h.resident_step_enqueue(dt, warmup + i)
                if after_step:
                    after_step(mode, i)

            us, w = tick_us(stream, ticks, tick, wall=True)
            times[name].append(us)
            wall[name].append(w)
            kernel[name] = h.last_kernel()
            if check:
                check(mode, kernel[name])
    return times, wall, kernel


def closed_loop(bat, path, s0, seeds, dt, ticks, extra, timed=False):
    """the closed-loop leg of a fresh handle: all its robots on `path` from s0 for `ticks` resident ticks, then per robot
    {"finite", "max_m", "rms_m"} of its trace (tracking_errors) and the tool's extra(b, trace, finite) fields; with `timed`,
    (that, us per tick between two events on the idle default stream, the synchronisation included)"""
    bat.resident_set_paths(path)
    bat.resident_set_poses(s0, seeds)
    if timed:
        start, stop, elapsed_us = event_pair(None, idle_device=True)
        start()
    for i in range(ticks):
        bat.resident_step_enqueue(dt, i, advance=i > 0)
    bat.synchronize()
    if timed:
        stop()
    out = []
    for b in range(len(s0)):
        tr = bat.resident_read_trace(b)
        finite = bool(np.all(np.isfinite(tr)))
        mx, rms = tracking_errors(tr, *path) if finite else (float("nan"), float("nan"))
        out.append({"finite": finite, "max_m": mx, "rms_m": rms, **extra(b, tr, finite)})
    return (out, elapsed_us() / ticks) if timed else out


# ---- summaries -------------------------------------------------------------------------------------------------------------------
def stats(v, baseline=False):
    out = {"median": float(np.median(v)), "rounds": [float(x) for x in v]}
    if baseline:
        out["spread"] = float(max(v) - min(v))
    return out


def summary(res, times, unit, baseline="off"):
    """into res: the rounds under "per_round", the median of every key of `times`, and the spread of the keys that begin with
    `baseline`, every name with `unit` appended"""
    res["per_round"] = {k + unit: v for k, v in times.items()}
    for k, v in times.items():
        res[k + unit] = float(np.median(v))
        if baseline and k.startswith(baseline):
            res["spread_" + k + unit] = float(max(v) - min(v))


def tick_stats(out, times, wall, baseline="none"):
    """into out: the costmap family's name_tick_us and name_wall_us, each a stats"""
    for name in times:
        out[name + "_tick_us"] = stats(times[name], name == baseline)
        out[name + "_wall_us"] = stats(wall[name], name == baseline)


def shape(p, B):
    return {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B}


# ---- the document tail -----------------------------------------------------------------------------------------------------------
def parser(out, iters=None, ticks=None, rounds=3, warmup=20):
    """the tools' command line; --iters and --ticks exist where a default is given, --out defaults to profiles/<out>"""
    ap = argparse.ArgumentParser()
    if iters:
        ap.add_argument("--iters", type=int, default=iters, help="timed launches per round (>= 256 for the kernel figure)")
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--warmup", type=int, default=warmup)
    if ticks:
        ap.add_argument("--ticks", type=int, default=ticks, help="timed ticks per round and mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out) if out else None)
    return ap


def header():
    import torch
    props = torch.cuda.get_device_properties(0)
    return {"device": props.name, "cus": props.multi_processor_count}


def new_stream():
    import torch
    return torch.cuda.Stream()


def emit(out, path):
    """print the document, and write it to `path` if given"""
    text = json.dumps(out, indent=1)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")

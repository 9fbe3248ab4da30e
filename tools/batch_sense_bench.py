#!/usr/bin/env python3
"""The simulated range sensor (ccv_mppi_batch_resident_sense_enqueue) against what a caller of the parent
commit has to do to give a resident fleet sensor data: `python tools/batch_sense_bench.py [--out FILE]` (default
profiles/batch_sense_bench.json).  The method of tools/batch_scan_bench.py: medians of --rounds rounds beside the max - min of the
baseline's rounds.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 map per robot placed round its start pose, R = 6, one world
under all of them (2 % occupied), 360 beams of reach 99: `none`, no sensing; `sense`, all 64 robots sense after every tick, in
one call; `host_cast`, the parent's only way: _resident_read (a flush and a synchronisation), the checker's vectorised cast per
robot on the host (tests/sense_reference.py), one _scan_occupancy_enqueue of the 64 maps.  Device events around --ticks ticks,
us per tick, and the wall time of the same loop; `sense_call_us`, the host time of one sense call of the 64 robots with the
stream idle and a staging slot free.  The robots drive 1.6 cells a tick: warm-up and ticks together stay under the 100 cells
from a map's centre to its edge, so every sensor cell stays inside its map (the scan call refuses one outside).

One robot with 4 096 beams of reach 600 in a 4 000 x 3 000 world (0.2 % occupied) and a map of its size at R = 6 -- one
workgroup casts them all: `sense_ms`, the wall time of the call and a synchronisation, and `sense_kernels_us`, the two launches
between two events.  One JSON document goes to stdout (and --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402
import sense_reference as SN  # noqa: E402
from batch_costmap_bench import layer, stats  # noqa: E402
from batch_obstacles_bench import fleet  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "sense", "host_cast")
TICK_R, TICK_N, TICK_BEAMS, TICK_REACH = 6, 200, 360, 99
BIG, BIG_R, BIG_BEAMS, BIG_REACH = (4000, 3000), 6, 4096, 600
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def raw_sense(h, inst, beams):
    rc = h.lib.ccv_mppi_batch_resident_sense_enqueue(h._h, len(inst), inst.ctypes.data_as(i32p), len(beams), beams.ctypes.data_as(i32p), 0, 255)
    assert rc == capi.OK, rc


def cast_host(world, threshold, s, beams):
    """(ends int32 [n][2] in world cells, hits uint8 [n]) of one robot: the blocked cell of a blocked beam, else its end cell"""
    first = SN.sense_vectorised(world, threshold, s, beams)
    d = beams.astype(np.int64)
    ad = np.abs(d)
    xmajor = ad[:, 0] >= ad[:, 1]
    a, b = np.where(xmajor, ad[:, 0], ad[:, 1]), np.where(xmajor, ad[:, 1], ad[:, 0])
    i = np.where(first >= 0, first, a)
    minor = (2 * i * b + a) // np.maximum(2 * a, 1)
    sg = np.where(d < 0, -1, 1)
    x = s[0] + sg[:, 0] * np.where(xmajor, i, minor)
    y = s[1] + sg[:, 1] * np.where(xmajor, minor, i)
    return np.stack([x, y], axis=1), (first >= 0).astype(np.uint8)


def resident_tick(ticks, rounds, warmup):
    import torch
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = fleet(p, B)
    infl = batch.inflation_profile(TICK_R * res, res)
    assert infl[0] == TICK_R and (warmup + ticks) * p.v_ref * p.dt / res < n // 2
    origin = (float(np.floor(s0[:, 0].min()) - 12.0), float(np.floor(s0[:, 1].min()) - 12.0))
    wnx, wny = int((s0[:, 0].max() + 24.0 - origin[0]) / res), int((s0[:, 1].max() + 24.0 - origin[1]) / res)
    world = layer(wnx, wny, seed=4)
    cell0 = [SN.pose_cell(s0[b, 0], s0[b, 1], origin, res, wnx, wny) for b in range(B)]
    anchors = np.array([(c[0] - n // 2, c[1] - n // 2) for c in cell0], dtype=np.int32)
    occ = [(np.zeros((n, n), dtype=np.uint8), (origin[0] + anchors[b, 0] * res, origin[1] + anchors[b, 1] * res), res, 0.0, 128) for b in range(B)]
    beams = batch.beam_fan(TICK_BEAMS, TICK_REACH)
    inst = np.arange(B, dtype=np.int32)
    map_of = np.arange(B, dtype=np.int32)
    n_rays = np.full(B, TICK_BEAMS, dtype=np.int32)
    stream = torch.cuda.Stream()
    h = amd.BatchController([p] * B, B, min_shift=True)
    h.set_stream(stream.cuda_stream)
    h.resident_set_paths(paths)
    times = {m: [] for m in TICK_MODES}
    wall = {m: [] for m in TICK_MODES}
    for _r in range(rounds):
        for mode in TICK_MODES:
            h.set_occupancy(occ, infl, map_of, W_GRID)
            h.set_world(world, 128, origin, res, anchors, TICK_BEAMS)
            h.resident_set_poses(s0, seeds)   # (every round from the start poses)
            for i in range(warmup):
                h.resident_step_enqueue(p.dt, i, advance=i > 0)
            h.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record(stream)
            for i in range(ticks):
                h.resident_step_enqueue(p.dt, warmup + i)
                if mode == "sense":
                    raw_sense(h, inst, beams)
                elif mode == "host_cast":
                    pose = h.resident_read()[0]
                    sensors, ends, hits = [], [], []
                    for b in range(B):
                        s = SN.pose_cell(pose[b, 0], pose[b, 1], origin, res, wnx, wny)
                        e, hit = cast_host(world, 128, s, beams)
                        sensors.append((s[0] - anchors[b, 0], s[1] - anchors[b, 1]))
                        ends.append(e - anchors[b])
                        hits.append(hit)
                    sensors = np.ascontiguousarray(sensors, dtype=np.int32)
                    end_xy = np.ascontiguousarray(np.concatenate(ends), dtype=np.int32)
                    hit = np.ascontiguousarray(np.concatenate(hits))
                    rc = h.lib.ccv_mppi_batch_scan_occupancy_enqueue(h._h, B, map_of.ctypes.data_as(i32p), sensors.ctypes.data_as(i32p), n_rays.ctypes.data_as(i32p),
                                                                     end_xy.ctypes.data_as(i32p), hit.ctypes.data_as(u8p), 0, 255)
                    assert rc == capi.OK, rc
            stop.record(stream)
            stop.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e6 / ticks)
            times[mode].append(start.elapsed_time(stop) * 1e3 / ticks)
            assert h.last_kernel() & capi.BATCH_KERNEL_GRID
            if mode != "none":
                assert max(int(h.read_occupancy(b).max()) for b in (0, B - 1)) == 255, "nothing was marked"
    # the host time of the call itself: stream idle, slots free (fewer calls than slots between two synchronisations)
    call = []
    for _r in range(8 * rounds):
        h.synchronize()
        t0 = time.perf_counter()
        for i in range(capi.OCC_PATCH_SLOTS - 1):
            raw_sense(h, inst, beams)
        call.append((time.perf_counter() - t0) * 1e6 / (capi.OCC_PATCH_SLOTS - 1))
    h.close()
    out = {"model": p.model, "K": p.num_samples, "H": p.horizon, "B": B, "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks, "warmup": warmup,
           "world": [wnx, wny], "sense": "%d beams of reach %d per robot, one call for all robots" % (TICK_BEAMS, TICK_REACH)}
    out["sense_call_us"] = stats(call[rounds:])
    for mode in TICK_MODES:
        out[mode + "_tick_us"] = stats(times[mode], mode == "none")
        out[mode + "_wall_us"] = stats(wall[mode], mode == "none")
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  sense %.2f / %.2f  host_cast %.2f / %.2f; "
          "one sense call of 64 robots %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["sense_tick_us"]["median"],
             out["sense_wall_us"]["median"], out["host_cast_tick_us"]["median"], out["host_cast_wall_us"]["median"],
             out["sense_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def big_world(rounds):
    import torch
    nx, ny = BIG
    p = configs.diff_drive_defaults(128, 15)
    h = amd.BatchController(p, 1)
    infl = batch.inflation_profile(BIG_R * RESOLUTION, RESOLUTION)
    assert infl[0] == BIG_R
    h.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), (0.0, 0.0), RESOLUTION, 0.0, 128)], infl, [0], W_GRID)
    world = np.where(np.random.default_rng(6).random((ny, nx)) < 0.002, 255, 0).astype(np.uint8)
    h.set_world(world, 128, (0.0, 0.0), RESOLUTION, [(0, 0)], BIG_BEAMS)
    h.resident_set_paths(amd.make_path("dkan"))
    h.resident_set_poses(np.array([[(nx // 2 + 0.5) * RESOLUTION, (ny // 2 + 0.5) * RESOLUTION, 0.0]]), 1)
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    inst, beams = np.zeros(1, dtype=np.int32), batch.beam_fan(BIG_BEAMS, BIG_REACH)
    raw_sense(h, inst, beams)   # (warm-up)
    h.synchronize()
    first = h.resident_read_sense()[0][0]
    wall, kern = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        raw_sense(h, inst, beams)
        h.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        raw_sense(h, inst, beams)
        stop.record(stream)
        stop.synchronize()
        kern.append(start.elapsed_time(stop) * 1e3)
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "beams": BIG_BEAMS, "reach": BIG_REACH, "blocked": int((first >= 0).sum()),
           "mean_cells_searched": float(np.where(first >= 0, first, BIG_REACH).mean()), "sense_ms": stats(wall), "sense_kernels_us": stats(kern)}
    print("4000 x 3000 R=6, one robot, 4096 beams of reach 600 (%d blocked): call and synchronisation %.3f ms, kernels %.1f us"
          % (out["blocked"], out["sense_ms"]["median"], out["sense_kernels_us"]["median"]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_sense_bench.json"))
    args = ap.parse_args()
    import torch
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "cus": props.multi_processor_count, "resident": resident_tick(args.ticks, args.rounds, args.warmup),
           "big_world": big_world(args.rounds)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

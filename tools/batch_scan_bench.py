#!/usr/bin/env python3
"""Scan tracing (ccv_mppi_batch_scan_occupancy_enqueue) against what a caller of the parent commit has to do
with a range scan: `python tools/batch_scan_bench.py [--out FILE]` (default profiles/batch_scan_bench.json).  The method and the
resident loop (its costmap form) are those of tools/bench_support.py.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 200 x 200 map per robot, R = 6: `none`, no map change; `scan`, all 64
maps scanned with 360 rays each from the map's centre after every tick, in one call (ends and hits prepared beforehand: what is
charged is the call); `host_trace`, the parent's only way: per map the rays traced with numpy into the host's copy of the layer
and the bounding box sent with one _update_occupancy_enqueue.  Device events around --ticks ticks, us per tick, and the wall time
of the same loop; `scan_call_us`, the host time of one scan call of the 64 maps with the stream idle and a staging slot free.

One 4 000 x 3 000 map at R = 6 with 2 000 rays of reach about 600 in one entry -- one workgroup traces them all: `scan_ms`, the
wall time of the call and a synchronisation, and `scan_kernels_us`, the two launches between two events.  One JSON document goes
to stdout (and --out)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)
import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "scan", "host_trace")
TICK_R, TICK_N, TICK_RAYS = 6, 200, 360
BIG, BIG_R, BIG_RAYS, BIG_REACH = (4000, 3000), 6, 2000, 600
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def scan_of(sensor, n, lo, hi, seed):
    """(ends int32 [n][2], hits uint8 [n]): n beams all round, ranges uniform in [lo, hi) cells, 70 % of them hits"""
    rng = np.random.default_rng(seed)
    t, r = 2.0 * np.pi * np.arange(n) / n, rng.uniform(lo, hi, n)
    ends = np.stack([sensor[0] + np.rint(r * np.cos(t)), sensor[1] + np.rint(r * np.sin(t))], axis=1).astype(np.int32)
    return np.ascontiguousarray(ends), (rng.random(n) < 0.7).astype(np.uint8)


def trace_host(cells, sensor, ends, hits, clear=0, mark=255):
    """the call's spec with numpy, all rays of an entry at once, in place -> the bounding box (x0, y0, w, h) of what it touched.
    The closed form and the box are those of tests/scan_reference.py (ray_cells, scan_box), which takes one ray at a time: this
    is the vectorised form a caller of the parent would write, and its cost is what mode `host_trace` charges."""
    ny, nx = cells.shape
    d = ends.astype(np.int64) - np.asarray(sensor, dtype=np.int64)
    ad = np.abs(d)
    xmajor = ad[:, 0] >= ad[:, 1]
    a, b = np.where(xmajor, ad[:, 0], ad[:, 1]), np.where(xmajor, ad[:, 1], ad[:, 0])
    i = np.arange(int(a.max()) if len(a) else 0, dtype=np.int64)[None, :]
    minor = (2 * i * b[:, None] + a[:, None]) // np.maximum(2 * a[:, None], 1)
    sg = np.where(d < 0, -1, 1)
    x = sensor[0] + sg[:, :1] * np.where(xmajor[:, None], i, minor)
    y = sensor[1] + sg[:, 1:] * np.where(xmajor[:, None], minor, i)
    ok = (i < a[:, None]) & (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
    cells[y[ok], x[ok]] = clear
    e = ends[hits != 0]
    e = e[(e[:, 0] >= 0) & (e[:, 0] < nx) & (e[:, 1] >= 0) & (e[:, 1] < ny)]
    cells[e[:, 1], e[:, 0]] = mark
    x0, y0 = max(min(int(ends[:, 0].min()), sensor[0]), 0), max(min(int(ends[:, 1].min()), sensor[1]), 0)
    x1, y1 = min(max(int(ends[:, 0].max()), sensor[0]) + 1, nx), min(max(int(ends[:, 1].max()), sensor[1]) + 1, ny)
    return x0, y0, x1 - x0, y1 - y0


def raw_scan(h, maps, sensors, n_rays, end_xy, hit):
    rc = h.lib.ccv_mppi_batch_scan_occupancy_enqueue(h._h, len(maps), maps.ctypes.data_as(i32p), sensors.ctypes.data_as(i32p), n_rays.ctypes.data_as(i32p),
                                                     end_xy.ctypes.data_as(i32p), hit.ctypes.data_as(u8p), 0, 255)
    assert rc == capi.OK, rc


def resident_tick(ticks, rounds, warmup):
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(TICK_R, res)
    cells = [bs.layer(n, n, seed=20 + b) for b in range(B)]
    occ = [(cells[b], (s0[b, 0] - 0.5 * n * res, s0[b, 1] - 0.5 * n * res), res, 0.0, 128) for b in range(B)]
    sensor = (n // 2, n // 2)
    per_map = [[scan_of(sensor, TICK_RAYS, 40, 99, 1000 * phase + b) for b in range(B)] for phase in range(16)]
    maps, sensors = np.arange(B, dtype=np.int32), np.ascontiguousarray(np.tile(np.array(sensor, dtype=np.int32), (B, 1)))
    n_rays = np.full(B, TICK_RAYS, dtype=np.int32)
    calls = [(maps, sensors, n_rays, np.ascontiguousarray(np.concatenate([e for e, _ in ph])), np.ascontiguousarray(np.concatenate([h for _, h in ph])))
             for ph in per_map]
    map_of = np.arange(B, dtype=np.int32)
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)
    mirror = []   # (the host's copy of the layers, which mode `host_trace` needs)

    def set_mode(h, _mode):
        h.set_occupancy(occ, infl, map_of, W_GRID)
        mirror[:] = [c.copy() for c in cells]

    def after_step(mode, i):
        if mode == "scan":
            raw_scan(h, *calls[i % 16])
        elif mode == "host_trace":
            for b in range(B):
                ends, hits = per_map[i % 16][b]
                x0, y0, bw, bh = trace_host(mirror[b], sensor, ends, hits)
                h.update_occupancy(b, x0, y0, mirror[b][y0:y0 + bh, x0:x0 + bw])

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup,
                                             after_step=after_step, costmap_form=True, check=bs.check_grid)
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks,
           "scan": "%d rays per map from the centre, ranges 40 .. 99 cells, 70 %% hits, one call for all maps" % TICK_RAYS,
           "scan_call_us": bs.idle_call_us(h, lambda i: raw_scan(h, *calls[i]), rounds)}
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  scan %.2f / %.2f  host_trace %.2f / %.2f; "
          "one scan call of 64 maps %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["scan_tick_us"]["median"],
             out["scan_wall_us"]["median"], out["host_trace_tick_us"]["median"], out["host_trace_wall_us"]["median"],
             out["scan_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def big_map(rounds):
    nx, ny = BIG
    h = amd.BatchController(configs.diff_drive_defaults(128, 15), 1)
    h.set_occupancy([(bs.layer(nx, ny), (0.0, 0.0), RESOLUTION, 0.0, 128)], bs.inflation(BIG_R, RESOLUTION), [0], W_GRID)
    stream = bs.new_stream()
    h.set_stream(stream.cuda_stream)
    sensor = (nx // 2, ny // 2)
    ends, hits = scan_of(sensor, BIG_RAYS, BIG_REACH - 50, BIG_REACH + 50, 5)
    args = (np.zeros(1, dtype=np.int32), np.array([sensor], dtype=np.int32), np.full(1, BIG_RAYS, dtype=np.int32), ends, hits)
    raw_scan(h, *args)   # (warm-up)
    h.synchronize()
    scan_ms, kernels_us = bs.one_call_ms_and_us(h, stream, rounds, lambda: raw_scan(h, *args))
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "rays": BIG_RAYS, "reach": BIG_REACH, "scan_ms": scan_ms, "scan_kernels_us": kernels_us}
    print("4000 x 3000 R=6, one entry of 2000 rays of reach 600: call and synchronisation %.3f ms, kernels %.1f us"
          % (out["scan_ms"]["median"], out["scan_kernels_us"]["median"]), file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_scan_bench.json", ticks=256).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "big_map": big_map(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

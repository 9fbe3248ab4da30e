#!/usr/bin/env python3
"""The simulated range sensor (ccv_mppi_batch_resident_sense_enqueue) against what a caller of the parent
commit has to do to give a resident fleet sensor data: `python tools/batch_sense_bench.py [--out FILE]` (default
profiles/batch_sense_bench.json).  The method and the resident loop (its costmap form) are those of tools/bench_support.py.

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
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(bs.ROOT, "tests"))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
from ccv_mppi_path_tracker_amd import batch, capi, configs  # noqa: E402
import sense_reference as SN  # noqa: E402

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
    """(ends int32 [n][2] in world cells, hits uint8 [n]) of one robot: the blocked cell of a blocked beam, else its end cell.
    The cast is the reference's; the one cell per beam below is its closed form (tests/sense_reference.py, beam_cells, which
    lists every cell of one beam) for all beams at once, as a caller of the parent would write it: mode `host_cast` charges it."""
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
    p, B, n, res = configs.diff_drive_defaults(1000, 15), 64, TICK_N, RESOLUTION
    paths, s0, seeds = bs.fleet(p, B)
    infl = bs.inflation(TICK_R, res)
    assert (warmup + ticks) * p.v_ref * p.dt / res < n // 2
    origin = (float(np.floor(s0[:, 0].min()) - 12.0), float(np.floor(s0[:, 1].min()) - 12.0))
    wnx, wny = int((s0[:, 0].max() + 24.0 - origin[0]) / res), int((s0[:, 1].max() + 24.0 - origin[1]) / res)
    world = bs.layer(wnx, wny, seed=4)
    cell0 = [SN.pose_cell(s0[b, 0], s0[b, 1], origin, res, wnx, wny) for b in range(B)]
    anchors = np.array([(c[0] - n // 2, c[1] - n // 2) for c in cell0], dtype=np.int32)
    occ = [(np.zeros((n, n), dtype=np.uint8), (origin[0] + anchors[b, 0] * res, origin[1] + anchors[b, 1] * res), res, 0.0, 128) for b in range(B)]
    beams = batch.beam_fan(TICK_BEAMS, TICK_REACH)
    inst = np.arange(B, dtype=np.int32)
    map_of = np.arange(B, dtype=np.int32)
    n_rays = np.full(B, TICK_BEAMS, dtype=np.int32)
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)

    def set_mode(h, _mode):
        h.set_occupancy(occ, infl, map_of, W_GRID)
        h.set_world(world, 128, origin, res, anchors, TICK_BEAMS)

    def after_step(mode, _i):
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

    def check(mode, kernel):
        bs.check_grid(mode, kernel)
        if mode != "none":
            assert max(int(h.read_occupancy(b).max()) for b in (0, B - 1)) == 255, "nothing was marked"

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup,
                                             after_step=after_step, costmap_form=True, check=check)
    out = {**bs.shape(p, B), "maps": B, "map": [n, n], "R": TICK_R, "ticks": ticks, "warmup": warmup, "world": [wnx, wny],
           "sense": "%d beams of reach %d per robot, one call for all robots" % (TICK_BEAMS, TICK_REACH),
           "sense_call_us": bs.idle_call_us(h, lambda _i: raw_sense(h, inst, beams), rounds)}
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  sense %.2f / %.2f  host_cast %.2f / %.2f; "
          "one sense call of 64 robots %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["sense_tick_us"]["median"],
             out["sense_wall_us"]["median"], out["host_cast_tick_us"]["median"], out["host_cast_wall_us"]["median"],
             out["sense_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def big_world(rounds):
    nx, ny = BIG
    p = configs.diff_drive_defaults(128, 15)
    h = amd.BatchController(p, 1)
    h.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), (0.0, 0.0), RESOLUTION, 0.0, 128)], bs.inflation(BIG_R, RESOLUTION), [0], W_GRID)
    world = np.where(np.random.default_rng(6).random((ny, nx)) < 0.002, 255, 0).astype(np.uint8)
    h.set_world(world, 128, (0.0, 0.0), RESOLUTION, [(0, 0)], BIG_BEAMS)
    h.resident_set_paths(amd.make_path("dkan"))
    h.resident_set_poses(np.array([[(nx // 2 + 0.5) * RESOLUTION, (ny // 2 + 0.5) * RESOLUTION, 0.0]]), 1)
    stream = bs.new_stream()
    h.set_stream(stream.cuda_stream)
    inst, beams = np.zeros(1, dtype=np.int32), batch.beam_fan(BIG_BEAMS, BIG_REACH)
    raw_sense(h, inst, beams)   # (warm-up)
    h.synchronize()
    first = h.resident_read_sense()[0][0]
    sense_ms, kernels_us = bs.one_call_ms_and_us(h, stream, rounds, lambda: raw_sense(h, inst, beams))
    h.close()
    out = {"nx": nx, "ny": ny, "R": BIG_R, "beams": BIG_BEAMS, "reach": BIG_REACH, "blocked": int((first >= 0).sum()),
           "mean_cells_searched": float(np.where(first >= 0, first, BIG_REACH).mean()), "sense_ms": sense_ms, "sense_kernels_us": kernels_us}
    print("4000 x 3000 R=6, one robot, 4096 beams of reach 600 (%d blocked): call and synchronisation %.3f ms, kernels %.1f us"
          % (out["blocked"], out["sense_ms"]["median"], out["sense_kernels_us"]["median"]), file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_sense_bench.json", ticks=40, warmup=10).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "big_world": big_world(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Costmaps inflated on the device (ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue) against what a
caller of the parent commit has to do: `python tools/batch_costmap_bench.py [--out FILE]` (default
profiles/batch_costmap_bench.json).  The method and the resident loop (its costmap form) are those of tools/bench_support.py.

Full inflation, 400 x 300 and 4 000 x 3 000 cells at R = 3 and R = 20, 2 % of the cells occupied: `device_ms`, the wall time of
one _set_occupancy (checks, allocation, upload of the uint8 layer, one k_inflate launch, synchronisation); `host_ms`, the
baseline: the numpy checker (tests/costmap_reference.py, the separable form) on the host plus one _set_grids with its float map;
`kernels_us` (400 x 300 only: a whole-map patch is within CCV_MPPI_OCC_PATCH_MAX_CELLS), the patch writer and k_inflate over the
whole map between two events.

Resident tick, diff drive K = 1 000, H = 15, B = 64, one 400 x 300 map shared by all instances, R = 6: `none`, no map updates;
`patch`, one 64 x 64 patch enqueued after every tick; `patch_1x1`, a patch of one cell (the floor: two more launches of one workgroup
each); `set_grids`, the parent's only way, a full _set_grids before every tick
(the map itself precomputed: only the upload is charged).  Device events around --ticks ticks, us per tick, and the wall
time of the same loop; `patch_call_us`, the host time of one _update_occupancy_enqueue call with the stream idle and a staging slot
free (what the call costs the thread that makes it).  One JSON document goes to stdout (and --out)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_support as bs  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, os.path.join(bs.ROOT, "tests"))

import ccv_mppi_path_tracker_amd as amd  # noqa: E402
import costmap_reference as CR  # noqa: E402
from ccv_mppi_path_tracker_amd import capi, configs  # noqa: E402

SIZES = ((400, 300), (4000, 3000))
RADII = (3, 20)
RESOLUTION = 0.05
W_GRID = 0.01
TICK_MODES = ("none", "patch", "patch_1x1", "set_grids")
TICK_R, PATCH = 6, 64


def full_inflation(rounds):
    h = amd.BatchController(configs.diff_drive_defaults(128, 15), 1)
    out = []
    for nx, ny in SIZES:
        cells = bs.layer(nx, ny)
        for R in RADII:
            infl = bs.inflation(R, RESOLUTION)
            occ = [(cells, (0.0, 0.0), RESOLUTION, 0.0, 128)]
            h.set_occupancy(occ, infl, [0], W_GRID)   # (warm-up)
            dev, host, kern = [], [], []
            for _ in range(rounds):
                dev.append(bs.wall_us(lambda: h.set_occupancy(occ, infl, [0], W_GRID))[0] * 1e-3)
                if nx * ny <= capi.OCC_PATCH_MAX_CELLS:
                    stream = bs.new_stream()
                    h.set_stream(stream.cuda_stream)
                    kern.append(bs.tick_us(stream, 1, lambda _i: h.update_occupancy(0, 0, 0, cells)))
                    h.set_stream(0)
            got = h.get_grids()[0][0][0]

            def on_host():
                cost = CR.cost_separable(cells, 128, *infl)
                h.set_grids([(cost, (0.0, 0.0), RESOLUTION, 0.0)], [0], W_GRID)
                return cost

            for _ in range(rounds):
                us, cost = bs.wall_us(on_host)
                host.append(us * 1e-3)
            assert got.tobytes() == cost.tobytes()
            r = {"nx": nx, "ny": ny, "R": R, "device_ms": bs.stats(dev), "host_ms": bs.stats(host, True)}
            if kern:
                r["kernels_us"] = bs.stats(kern)
            out.append(r)
            print("inflation %4d x %4d R=%2d: device %.2f ms, host %.1f ms (spread %.1f)%s"
                  % (nx, ny, R, r["device_ms"]["median"], r["host_ms"]["median"], r["host_ms"]["spread"],
                     ", kernels %.1f us" % r["kernels_us"]["median"] if kern else ""), file=sys.stderr, flush=True)
    h.close()
    return out


def resident_tick(ticks, rounds, warmup):
    p, B = configs.diff_drive_defaults(1000, 15), 64
    nx, ny = SIZES[0]
    paths, s0, seeds = bs.fleet(p, B)
    xs, ys = np.concatenate([q[0] for q in paths]), np.concatenate([q[1] for q in paths])
    lo_x, hi_x, lo_y, hi_y = float(xs.min()) - 3.0, float(xs.max()) + 3.0, float(ys.min()) - 3.0, float(ys.max()) + 3.0
    res = max((hi_x - lo_x) / nx, (hi_y - lo_y) / ny)
    cells = bs.layer(nx, ny)
    infl = bs.inflation(TICK_R, res)
    cost = CR.cost_separable(cells, 128, *infl)
    rng = np.random.default_rng(3)
    patches = [(int(rng.integers(0, nx - PATCH)), int(rng.integers(0, ny - PATCH)), np.where(rng.random((PATCH, PATCH)) < 0.02, 255, 0).astype(np.uint8))
               for _ in range(16)]
    one = np.full((1, 1), 255, dtype=np.uint8)
    stream = bs.new_stream()
    h = bs.resident_handle([p] * B, B, stream, paths, min_shift=True)
    whole_map = [(cost, (lo_x, lo_y), res, 0.0)]

    def set_mode(h, mode):
        if mode == "set_grids":
            h.set_grids(whole_map, 0, W_GRID)
        else:
            h.set_occupancy([(cells, (lo_x, lo_y), res, 0.0, 128)], infl, 0, W_GRID)

    def before_step(mode, _i):
        if mode == "set_grids":
            h.set_grids(whole_map, 0, W_GRID)

    def after_step(mode, i):
        if mode == "patch":
            h.update_occupancy(0, *patches[i % len(patches)])
        elif mode == "patch_1x1":
            h.update_occupancy(0, patches[i % len(patches)][0], patches[i % len(patches)][1], one)

    times, wall, _kernel = bs.resident_modes(h, stream, s0, seeds, p.dt, TICK_MODES, set_mode, ticks, rounds, warmup, before_step,
                                             after_step, costmap_form=True, check=bs.check_grid)
    set_mode(h, "none")
    out = {**bs.shape(p, B), "map": [nx, ny], "R": TICK_R, "patch": [PATCH, PATCH], "ticks": ticks,
           "patch_call_us": bs.idle_call_us(h, lambda i: h.update_occupancy(0, *patches[i]), rounds)}
    h.close()
    bs.tick_stats(out, times, wall)
    print("resident B=64 tick us (device events / wall): none %.2f / %.2f (spread %.2f)  patch %.2f / %.2f  patch 1 x 1 %.2f / %.2f  "
          "set_grids %.2f / %.2f; one patch call %.2f us of host time"
          % (out["none_tick_us"]["median"], out["none_wall_us"]["median"], out["none_tick_us"]["spread"], out["patch_tick_us"]["median"],
             out["patch_wall_us"]["median"], out["patch_1x1_tick_us"]["median"], out["patch_1x1_wall_us"]["median"],
             out["set_grids_tick_us"]["median"], out["set_grids_wall_us"]["median"], out["patch_call_us"]["median"]), file=sys.stderr, flush=True)
    return out


def main():
    args = bs.parser("batch_costmap_bench.json", ticks=256).parse_args()
    out = {**bs.header(), "resident": resident_tick(args.ticks, args.rounds, args.warmup), "inflation": full_inflation(args.rounds)}
    bs.emit(out, args.out)


if __name__ == "__main__":
    main()

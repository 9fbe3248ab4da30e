"""GPU tests (-m gpu) of the batch handles' scan tracing (ccv_mppi_batch_scan_occupancy_enqueue; BatchController.scan_occupancy;
DESIGN.md section 10n).

The contract is one sentence: after a call the layer and the float cells of a map are, in every bit, what a fresh _set_occupancy
of the scanned layer would produce.  The checker is tests/scan_reference.py on top of tests/costmap_reference.py -- integers and
one table lookup -- so everything is held against it with no tolerance, and a scanned handle against a twin that was given the
checker's float map through _set_grids bit for bit in everything a tick leaves.  No test asserts a time, and none checks from
the host that the call did not synchronise.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import batch_support as BS
import costmap_reference as CR
import costmap_support as CS
import fleet_support as FS
import grid_reference as GR
import obstacle_cases as OC
import roll_reference as RR
import scan_reference as SR
from batch_support import GRID, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import CLEAR_TICK, block_scans, derived, occ_map, same

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import costmap_door_cpu as CD  # noqa: E402

pytestmark = pytest.mark.gpu
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
FREE = CR.FREE_VALUE
CALL = "ccv_mppi_batch_scan_occupancy_enqueue"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.fixture(scope="module")
def small_handle():
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    yield bat
    bat.close()


def holds(bat, want):
    """want: per map (layer, threshold, R, profile, free_value), or None for a map not to look at"""
    grids = bat.get_grids()[0]
    assert len(grids) == len(want)
    for m, w in enumerate(want):
        if w is None:
            continue
        cells, threshold, R, profile, free = w
        assert same(bat.read_occupancy(m), cells), m
        assert same(grids[m][0], CR.cost_separable(cells, threshold, R, profile, free)), m


def raw_scan(bat, maps, sensors, ends, hits, clear=0, mark=255, expect=capi.OK):
    """the C call over the caller's own arrays, which are overwritten as soon as it returns"""
    maps = np.array(maps, dtype=np.int32)
    sensors = np.array(sensors, dtype=np.int32).reshape(-1, 2)
    n_rays = np.array([len(e) for e in ends], dtype=np.int32)
    end_xy = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.int32).reshape(-1, 2) for e in ends] + [np.zeros((0, 2), dtype=np.int32)]))
    hit = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.uint8).reshape(-1) for h in hits] + [np.zeros(0, dtype=np.uint8)]))
    rc = getattr(bat.lib, CALL)(bat._h, len(maps), maps.ctypes.data_as(i32p), sensors.ctypes.data_as(i32p), n_rays.ctypes.data_as(i32p),
                                end_xy.ctypes.data_as(i32p), hit.ctypes.data_as(u8p), clear, mark)
    assert rc == expect, (rc, bat.lib.ccv_mppi_batch_last_error(bat._h))
    maps[...] = -5
    sensors[...] = -7
    n_rays[...] = 1 << 30
    end_xy[...] = 12345
    hit[...] = 1 - (hit != 0)


# 1. one call against the checker ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 3, 17, 64))
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_one_call_equals_the_checker_from_scratch(small_handle, nx, ny, R):
    """the layers of the CPU list as the maps of one handle, all but the last scanned by one call per scan of the CPU list (map m
    takes scan k + m, so one call carries different scans); the layers accumulate from call to call"""
    bat, profile = small_handle, CR.distinct_profile(R)
    layers, scans = SR.layers(nx, ny), SR.scans(nx, ny)
    layers.append(("unnamed",) + layers[1][1:])
    bat.set_occupancy([occ_map(cells, threshold) for _, cells, threshold in layers], (R, profile, FREE), [0], 1.0)
    cells = [l[1] for l in layers]
    n = len(layers) - 1
    for k in range(len(scans)):
        picked = [scans[(k + m) % len(scans)] for m in range(n)]
        order = list(range(n))[::-1] if k % 2 else list(range(n))
        clear, mark = (0, 255) if k % 3 else (1, 254)
        bat.scan_occupancy(order, [picked[m][1] for m in order], [picked[m][2] for m in order], [picked[m][3] for m in order], clear=clear, mark=mark)
        for m in range(n):
            cells[m] = SR.apply_scan(cells[m], *picked[m][1:], clear=clear, mark=mark)
        holds(bat, [(cells[m], layers[m][2], R, profile, FREE) for m in range(n + 1)])
    assert same(cells[n], layers[n][1])


def test_a_fan_over_several_tiles_and_a_ray_of_the_longest_reach(small_handle):
    """193 x 129 at R = 64: the rectangle is three tiles by two and a cell more; 4097 x 3: one ray of reach 4096 from end to end"""
    bat, R, (nx, ny) = small_handle, 64, (193, 129)
    profile = CR.distinct_profile(R)
    rng = np.random.default_rng(7)
    cells = np.where(rng.random((ny, nx)) < 0.02, 200, 50).astype(np.uint8)
    cells[0, 0] = cells[ny - 1, nx - 1] = 200
    s = (60, 70)
    ends, hits = SR.fan(s, 720, 58.0, hit_every=40)
    bat.set_occupancy([occ_map(cells, 128)], (R, profile, FREE), [0], 1.0)
    bat.scan_occupancy([0], [s], [ends], [hits], clear=0, mark=255)
    new = SR.apply_scan(cells, s, ends, hits)
    assert len(np.unique(CR.cost_separable(new, 128, R, profile, FREE))) > 25 and not same(new, cells)
    holds(bat, [(new, 128, R, profile, FREE)])
    nx, ny, R = 4097, 3, 3
    profile = CR.distinct_profile(R)
    cells = np.full((ny, nx), 200, dtype=np.uint8)
    ends, hits = np.array([(4096, 2), (4096, 0), (-1000, 1)], dtype=np.int64), np.array([1, 0, 1], dtype=np.uint8)
    bat.set_occupancy([occ_map(cells, 128)], (R, profile, FREE), [0], 1.0)
    bat.scan_occupancy([0], [(0, 0)], [ends], [hits])
    new = SR.apply_scan(cells, (0, 0), ends, hits)
    assert new[0, :4096].max() == 0 and new[0, 4096] == 200 and new[2, 4096] == 255 and (new[2, :4096] == 0).sum() > 1000
    holds(bat, [(new, 128, R, profile, FREE)])
    with pytest.raises(RuntimeError):
        bat.scan_occupancy([0], [(0, 1)], [[(4097, 1)]], [[0]])


# 2. marks win over clears -------------------------------------------------------------------------------------------------------
def test_marks_win_over_clears_whatever_the_order():
    """1 024 rays through one cell, the sensor's right-hand neighbour, which is also the end of a hit in the middle of the list;
    the same rays reversed; two maps with the entries in either order"""
    nx, ny, R = 200, 150, 3
    profile = CR.distinct_profile(R)
    s, c = (20, 60), (21, 60)
    far = np.array([(s[0] + 100 + j, s[1] + k) for j in range(32) for k in range(-16, 16)], dtype=np.int64)
    assert len(far) == 1024 and all((SR.ray_cells(s, e)[1] == c).all() for e in far[::37])
    ends = np.concatenate([far[:512], np.array([c], dtype=np.int64), far[512:]])
    hits = np.zeros(len(ends), dtype=np.uint8)
    hits[512] = 1
    cells = np.full((ny, nx), 100, dtype=np.uint8)
    want = SR.apply_scan(cells, s, ends, hits, clear=0, mark=255)
    assert want[c[1], c[0]] == 255 and want[s[1], s[0]] == 0 and (want == 0).sum() > 2000
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    for rays, entries in (((ends, hits), [0, 1]), ((ends[::-1].copy(), hits[::-1].copy()), [0, 1]), ((ends, hits), [1, 0])):
        bat.set_occupancy([occ_map(cells, 100), occ_map(cells, 100)], (R, profile, FREE), [0], 1.0)
        # (map 1 gets the list rotated: the hit first)
        per = {0: rays, 1: (np.roll(rays[0], 512, axis=0), np.roll(rays[1], 512))}
        bat.scan_occupancy(entries, [s, s], [per[m][0] for m in entries], [per[m][1] for m in entries])
        holds(bat, [(want, 100, R, profile, FREE)] * 2)
    bat.close()


# 3. interleaved with patches and rolls ------------------------------------------------------------------------------------------
def test_scans_patches_and_rolls_back_to_back(small_handle):
    """a dozen scans, as many patches and six rolls with no synchronisation: 30 calls through a ring of CCV_MPPI_OCC_PATCH_SLOTS
    slots.  The caller's arrays are overwritten after each call; everything is read once, at the end.  A scan after a roll
    addresses the rolled frame: the checker applies every call to the layer as it stands."""
    bat = small_handle
    sizes, radii = [(150, 100), (67, 45)], [17, 3]
    rng = np.random.default_rng(12)
    cells = [np.where(rng.random((ny, nx)) < 0.3, 200, 50).astype(np.uint8) for nx, ny in sizes]
    infl = [(R, CR.distinct_profile(R), FREE) for R in radii]
    bat.set_occupancy([occ_map(c, 128) for c in cells], infl, [0], 1.0)
    bat.roll_occupancy([0, 1], 0, 0)   # the priming call: the rolls below allocate nothing
    assert 30 > capi.OCC_PATCH_SLOTS
    for i in range(12):
        maps = [1, 0] if i % 3 == 0 else [i % 2]
        sensors, ends, hits = [], [], []
        for m in maps:
            nx, ny = sizes[m]
            s = (int(rng.integers(0, nx)), int(rng.integers(0, ny)))
            e, h = SR.fan(s, int(rng.integers(1, 200)), float(rng.uniform(3, 80)), hit_every=int(rng.integers(0, 4)), phase=float(rng.uniform(0, 6)))
            cells[m] = SR.apply_scan(cells[m], s, e, h, clear=i, mark=255 - i)
            sensors.append(s), ends.append(e), hits.append(h)
        raw_scan(bat, maps, sensors, ends, hits, clear=i, mark=255 - i)
        m = (i + 1) % 2
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        x0, y0 = int(rng.integers(0, sizes[m][0] - w + 1)), int(rng.integers(0, sizes[m][1] - h + 1))
        patch = np.where(rng.random((h, w)) < 0.3, 200, 50).astype(np.uint8)
        cells[m] = CR.apply_patch(cells[m], x0, y0, patch)
        buf = patch.copy()
        bat.update_occupancy(m, x0, y0, buf)
        buf[...] = 255 - buf
        if i % 2 == 0:
            m = (i // 2) % 2
            dx, dy = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
            cells[m] = RR.roll_layer(cells[m], dx, dy, fill=200)
            bat.roll_occupancy([m], [dx], [dy], fill=200)
    holds(bat, [(cells[m], 128) + infl[m] for m in range(2)])


# 4. the same bits as a twin -----------------------------------------------------------------------------------------------------
INFLATION = CS.INFLATION


def scanned_twin_maps(geos, seed=0):
    """(set_occupancy's maps before the scan, the scans (sensor, ends, hits), the checker's float maps after it as set_grids takes
    them)"""
    R, profile, free = INFLATION
    occ, scans, flt = [], [], []
    for m, g in enumerate(geos):
        cells = CS.layer_like(g, seed + m)
        s = (g.nx // 2 + m, g.ny // 3)
        ends, hits = SR.fan(s, 180, 0.4 * max(g.nx, g.ny), hit_every=5, phase=0.3 * m)
        new = SR.apply_scan(cells, s, ends, hits)
        assert not same(new, cells)
        occ.append((cells, (g.ox, g.oy), g.resolution, float(g.outside), 128))
        scans.append((s, ends, hits))
        flt.append((CR.cost_separable(new, 128, R, profile, free), (g.ox, g.oy), g.resolution, float(g.outside)))
    return occ, scans, flt


def scan_all(bat, scans, order):
    bat.scan_occupancy(order, [scans[m][0] for m in order], [scans[m][1] for m in order], [scans[m][2] for m in order])


@pytest.mark.parametrize("shift,discs", [(False, "none"), (True, "none"), (False, "moving"), (True, "static")])
def test_a_scanned_handle_gives_the_bits_of_a_twin(shift, discs):
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, scans, flt = scanned_twin_maps(geos)
    d = OC.discs_for(p, inputs, ns=(32, 0, 3, 3, 32)) if discs != "none" else None
    vels = [np.stack([0.3 * np.cos(np.arange(len(a)) + b), 0.2 * np.sin(np.arange(len(a)) - b)], axis=1).reshape(-1, 2)
            for b, a in enumerate(d)] if discs == "moving" else None
    s0, rseeds = BS.start_poses(p, B)
    rgeos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    rocc, rscans, rflt = scanned_twin_maps(rgeos, seed=7)
    out = []
    for source in ("scanned", "grids"):
        bat = BatchController(p, B, min_shift=shift)
        if d is not None:
            bat.set_obstacles(d, OC.W_OBS, velocities=vels)
        if source == "scanned":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            bat.set_nominal(nom)
            bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)   # (a tick over the maps before the scan)
            k0 = bat.last_kernel()
            scan_all(bat, scans, [0, 1])
            assert bat.last_kernel() == k0
        else:
            bat.set_grids(flt, map_of, w)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res = [BS.snapshot(bat, u, st), bat.last_kernel(), derived(bat, 0), derived(bat, 1)]
        # five resident ticks over maps placed from the start poses
        if source == "scanned":
            bat.set_occupancy(rocc, INFLATION, map_of, w)
            scan_all(bat, rscans, [1, 0])
        else:
            bat.set_grids(rflt, map_of, w)
        bat.resident_set_paths([BS.path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, rseeds)
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(CS.tick_bits(bat) + [r.tobytes() for r in bat.resident_read()[:2]] + [bat.resident_read_trace(b).tobytes() for b in range(B)])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    a, b = out
    assert a[1] == b[1] == a[-1] == b[-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    assert same(a[2], b[2]) and same(a[3], b[3]) and len(np.unique(a[2])) > 5
    assert all(BS.same_bits(x, y) for x, y in zip(a[0], b[0]))
    for it in range(5):
        assert a[4 + it] == b[4 + it], it


def test_a_scanned_handle_gives_the_bits_of_a_twin_beside_the_fleet_term():
    p = FS.params("diff_drive", 1000, 15)
    B = 5
    s0, seeds, paths = FS.fleet_start(p, B)
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    occ, scans, flt = scanned_twin_maps(geos, seed=3)
    static = [FS.far_discs(b % 3, b) for b in range(B)]
    out = []
    for source in ("scanned", "grids"):
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0)))
        bat.resident_set_fleet_prediction(True)
        if source == "scanned":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            scan_all(bat, scans, [0, 1])
        else:
            bat.set_grids(flt, map_of, w)
        res = []
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(CS.tick_bits(bat) + [bat.resident_read()[0].tobytes()])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    assert out[0] == out[1] and out[0][-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT


# 5. stream order ----------------------------------------------------------------------------------------------------------------
T_STREAM = 30


def test_scans_take_effect_in_stream_order():
    """A: occupancy, one scan enqueued after every resident step and nothing else between the steps.  B: before every step the
    checker's full map of that moment through _set_grids.  B runs first, tick by tick, and places the scans: scan t leaves the
    cell of instance 0's pose after tick t (clipped to the map) for cells that a state of tick t read -- the obstacle is put
    ahead of the robot, in its fan -- marking every other one; every third scan only clears, a wider fan.  At least a third of
    the scans must change the cost of a cell that some covered state of tick t + 1 reads (on B's read-back candidates; A's are
    the same bits); the test fails there, before A runs, if the scene does not qualify."""
    p = configs.diff_drive_defaults(128, 15)
    B, R = 2, 3
    profile, free = CR.distinct_profile(R) * np.float32(0.001), 0.0   # (1.000 .. 1.009: the ring costs about what a cell does)
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    geo = GR.map_ahead(s0[0, :3], p.v_ref, p.dt, p.horizon, ahead=3.0)
    map_of, w = np.array([0, -1], dtype=np.int32), np.array([0.5, 0.0])
    inv = 1.0 / geo.resolution

    def result(bat):
        return [bat.get_nominal().tobytes(), bat.read_costs(0).tobytes(), bat.read_costs(1).tobytes(), bat.resident_read()[0].tobytes(),
                bat.resident_read_trace(0).tobytes(), bat.resident_read_trace(1).tobytes()]

    # B: the reference handle, which also places the scans
    cells = np.zeros((geo.ny, geo.nx), dtype=np.uint8)
    cost = CR.cost_separable(cells, 128, R, profile, free)
    ref = BatchController(p, B, min_shift=True)
    ref.resident_set_paths(paths)
    ref.resident_set_poses(s0, seeds)
    scans, changed, looked_at = [], None, 0
    for it in range(T_STREAM):
        ref.set_grids([(cost, (geo.ox, geo.oy), geo.resolution, float(geo.outside))], map_of, w)
        ref.resident_step_enqueue(p.dt, it, advance=it > 0)
        hit_cells = CS.cells_hit(geo, ref.read_candidates(0)[:, :GR.n_covered(p.model, p.horizon)])
        if changed is not None:
            looked_at += bool(np.intersect1d(hit_cells, changed).size)
        assert hit_cells.size > 0, "the fan left the map"
        pose = ref.resident_read()[0][0]
        s = (int(np.clip(np.floor((pose[0] - geo.ox) * inv), 0, geo.nx - 1)), int(np.clip(np.floor((pose[1] - geo.oy) * inv), 0, geo.ny - 1)))
        if it % 3 == 2:   # a clearing sweep over the cells read
            pick = hit_cells[::max(hit_cells.size // 60, 1)]
            hits = np.zeros(pick.size, dtype=np.uint8)
        else:             # obstacles in cells that states read
            pick = hit_cells[(7 * it + 3 + 17 * np.arange(6)) % hit_cells.size]
            hits = (np.arange(pick.size) % 2 == 0).astype(np.uint8)
        iy, ix = np.divmod(pick, geo.nx)
        ends = np.stack([ix, iy], axis=1).astype(np.int64)
        scans.append((s, ends, hits))
        cells = SR.apply_scan(cells, s, ends, hits)
        new = CR.cost_separable(cells, 128, R, profile, free)
        changed = np.flatnonzero(new.reshape(-1) != cost.reshape(-1))
        cost = new
    want, k_ref = result(ref), ref.last_kernel()
    ref.close()
    print("[stream order] %d of %d scans changed a cell that the next tick read" % (looked_at, T_STREAM - 1))
    assert 3 * looked_at >= T_STREAM
    # A: occupancy, scanned in stream order
    bat = BatchController(p, B, min_shift=True)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    bat.set_occupancy([(np.zeros((geo.ny, geo.nx), dtype=np.uint8), (geo.ox, geo.oy), geo.resolution, float(geo.outside), 128)],
                      (R, profile, free), map_of, w)
    for it in range(T_STREAM):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        raw_scan(bat, [0], [scans[it][0]], [scans[it][1]], [scans[it][2]])
    got = result(bat)
    assert bat.last_kernel() == k_ref == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    assert same(bat.read_occupancy(0), cells) and same(derived(bat), cost)
    bat.close()
    assert got == want


# 6. an obstacle appears in a scan and leaves in a later one -------------------------------------------------------------------------
def test_an_obstacle_appears_in_a_scan_and_leaves_in_a_later_one():
    """The door's scene (tools/costmap_door_cpu.py; tests/test_costmap_door_cpu.py holds its CPU restatement): the block is marked by
    a scan right after tick PATCH_TICK.  never: no scan -- some trace poses lie in the block's cells; marked: none do; cleared_by_scan: a
    clearing scan over the same cells right after tick CLEAR_TICK, when the robot has already turned away (its pose differs from
    never's); cleared_by_patch: the same history, and at that tick the block's cells zeroed by _update_occupancy_enqueue -- a run that
    sees no block from that tick on, with the same poses and seeds.  The last two are equal in every bit."""
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    s, marking, clearing = block_scans()
    x0, y0, patch = CD.block_patch()
    runs = {}
    for name in ("never", "marked", "cleared_by_scan", "cleared_by_patch"):
        bat = BatchController(p, 1, min_shift=True)
        bat.set_occupancy([(CD.empty_layer(), CD.ORIGIN, CD.RESOLUTION, 0.0, CD.THRESHOLD)], CD.inflation(), [0], CD.WEIGHT)
        bat.resident_set_paths([CD.GW.path()])
        bat.resident_set_poses(np.array([CD.START]), np.array([CD.SEED], dtype=np.uint64))
        for it in range(CD.TICKS):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if name != "never" and it == CD.PATCH_TICK:
                bat.scan_occupancy([0], [s], [marking[0]], [marking[1]])
            if name == "cleared_by_scan" and it == CLEAR_TICK:
                bat.scan_occupancy([0], [s], [clearing[0]], [clearing[1]])
            if name == "cleared_by_patch" and it == CLEAR_TICK:
                bat.update_occupancy(0, x0, y0, np.zeros_like(patch))
        trace = bat.resident_read_trace(0)
        assert len(trace) == CD.TICKS and bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
        runs[name] = (trace, bat.get_nominal().tobytes(), bat.read_costs(0).tobytes(), bat.read_occupancy(0), derived(bat))
        print("%s: %d poses in the block's cells, closest %.3f m, end x %.2f" % (name, CD.in_block(trace[:, :2]), CD.clearance(trace[:, :2]),
                                                                                  trace[-1, 0]))
        bat.close()
    assert CD.in_block(runs["never"][0][:, :2]) > 0
    assert CD.in_block(runs["marked"][0][:, :2]) == 0 and runs["marked"][3].max() == 255
    a, b = runs["cleared_by_scan"], runs["cleared_by_patch"]
    assert same(a[0][:CLEAR_TICK + 1], runs["marked"][0][:CLEAR_TICK + 1]) and not same(a[0][:CLEAR_TICK + 1], runs["never"][0][:CLEAR_TICK + 1])
    assert not same(a[0], runs["marked"][0])
    assert same(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and same(a[3], b[3]) and same(a[4], b[4])
    assert not a[3].any() and same(a[4], runs["never"][4])


# 7. plumbing --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls_change_nothing_and_the_setters_keep_the_scanned_map():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, scans, flt = scanned_twin_maps(geos)
    R, profile, free = INFLATION
    bat = BatchController(p, B)
    one_ray = ([[(3, 3)]], [[1]])
    # nothing set, and a caller's float maps: STATE
    raw_scan(bat, [0], [(1, 1)], *one_ray, expect=capi.ERR_STATE)
    bat.set_grids(flt, map_of, w)
    raw_scan(bat, [0], [(1, 1)], *one_ray, expect=capi.ERR_STATE)
    bat.set_occupancy(occ, INFLATION, map_of, w)

    def tick():
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        return BS.snapshot(bat, u, st, states=False)

    def state():
        return [bat.read_occupancy(m).tobytes() + derived(bat, m).tobytes() for m in range(2)] + [bat.get_occupancy()]

    scan_all(bat, scans, [1, 0])
    scanned = [(SR.apply_scan(occ[m][0], *scans[m]), 128, R, profile, np.float32(free)) for m in range(2)]
    holds(bat, scanned)
    before, bits = state(), tick()
    # calls of empty entries: nothing launched, nothing changed (more of them than the ring has slots: they take none)
    for _ in range(capi.OCC_PATCH_SLOTS + 2):
        raw_scan(bat, [0, 1], [(1, 1), (2, 2)], [[], []], [[], []])
        bat.scan_occupancy([1], [(0, 0)], [np.zeros((0, 2))], [np.zeros(0)])
    lib, ip = bat.lib, lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(i32p)   # noqa: E731
    assert getattr(lib, CALL)(bat._h, 1, ip([0]), ip([1, 1]), ip([0]), None, None, 0, 255) == capi.OK   # (no ray to read: no array needed)
    assert state() == before
    # every refusal
    nx, ny = geos[0].nx, geos[0].ny
    far = capi.SCAN_MAX_REACH + 1
    for maps, sensors, ends, hits, clear, mark in (
            ([], [], [], [], 0, 255), ([0, 1, 0], [(1, 1)] * 3, [[], [], []], [[], [], []], 0, 255),
            ([2], [(1, 1)], *one_ray, 0, 255), ([-1], [(1, 1)], *one_ray, 0, 255), ([1, 1], [(1, 1)] * 2, [[], []], [[], []], 0, 255),
            ([0], [(-1, 1)], *one_ray, 0, 255), ([0], [(1, -1)], *one_ray, 0, 255), ([0], [(nx, 1)], *one_ray, 0, 255), ([0], [(1, ny)], *one_ray, 0, 255),
            ([1, 0], [(1, 1), (nx, 0)], [[], []], [[], []], 0, 255),
            ([0], [(1, 1)], [[(1 + far, 1)]], [[0]], 0, 255), ([0], [(1, 1)], [[(1, 1 - far)]], [[1]], 0, 255),
            ([0], [(1, 1)], [[(2, 2), (-2 ** 31, 1)]], [[0, 0]], 0, 255), ([0], [(1, 1)], [[(2 ** 31 - 1, 2 ** 31 - 1)]], [[0]], 0, 255),
            ([0], [(1, 1)], *one_ray, -1, 255), ([0], [(1, 1)], *one_ray, 256, 255), ([0], [(1, 1)], *one_ray, 0, -1), ([0], [(1, 1)], *one_ray, 0, 256)):
        raw_scan(bat, maps, sensors, ends, hits, clear, mark, expect=capi.ERR_INVALID_ARG)
    e, h = np.array([3, 3], dtype=np.int32), np.ones(1, dtype=np.uint8)
    call = getattr(lib, CALL)
    assert call(bat._h, 1, ip([0]), ip([1, 1]), ip([-1]), e.ctypes.data_as(i32p), h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG   # a negative n_rays
    assert call(bat._h, 1, None, ip([1, 1]), ip([1]), e.ctypes.data_as(i32p), h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), None, ip([1]), e.ctypes.data_as(i32p), h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), ip([1, 1]), None, e.ctypes.data_as(i32p), h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), ip([1, 1]), ip([1]), None, h.ctypes.data_as(u8p), 0, 255) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), ip([1, 1]), ip([1]), e.ctypes.data_as(i32p), None, 0, 255) == capi.ERR_INVALID_ARG
    assert state() == before and all(BS.same_bits(a, b, states=False) for a, b in zip(bits, tick()))
    # the other setters keep the scanned map
    discs = OC.discs_for(p, inputs, ns=(0, 3, 0, 3, 0))
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_obstacles(discs, OC.W_OBS, velocities=[np.zeros((len(a), 2)) for a in discs])
    bat.set_obstacle_velocities(None)
    bat.set_obstacles(None)
    bat.set_min_shift(True)
    bat.set_min_shift(False)
    bat.resident_set_fleet(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0))
    bat.resident_set_fleet(None)
    holds(bat, scanned)
    assert state() == before and all(BS.same_bits(a, b, states=False) for a, b in zip(bits, tick()))
    # the float maps are a caller's again: no scan
    bat.set_grids(flt, map_of, w)
    raw_scan(bat, [0], [(1, 1)], *one_ray, expect=capi.ERR_STATE)
    bat.close()


def test_the_slot_size_limit():
    """tables and rays share one staging slot: one entry of 116 494 rays fits beside its 128 bytes of tables, one ray more does
    not.  The rays are 500 distinct ones over and over -- a ray traced twice changes nothing -- so the checker traces 500."""
    n = (capi.OCC_PATCH_MAX_CELLS - capi.SCAN_ENTRY_BYTES) // capi.SCAN_RAY_BYTES
    assert n == 116494
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    nx, ny, R = 200, 200, 3
    profile = CR.distinct_profile(R)
    cells = np.full((ny, nx), 200, dtype=np.uint8)
    s = (100, 90)
    ends500, hits500 = SR.fan(s, 500, 150.0, hit_every=9)
    ends, hits = np.resize(ends500, (n + 1, 2)), np.resize(hits500, n + 1)
    bat.set_occupancy([occ_map(cells, 128)], (R, profile, FREE), [0], 1.0)
    with pytest.raises(RuntimeError):
        bat.scan_occupancy([0], [s], [ends], [hits])
    assert bat.read_occupancy(0).min() == 200
    bat.scan_occupancy([0], [s], [ends[:n]], [hits[:n]])
    holds(bat, [(SR.apply_scan(cells, s, ends500, hits500), 128, R, profile, FREE)])
    # two entries: 2 * 128 bytes of tables
    bat.set_occupancy([occ_map(cells, 128), occ_map(cells, 128)], (R, profile, FREE), [0], 1.0)
    n2 = (capi.OCC_PATCH_MAX_CELLS - 2 * capi.SCAN_ENTRY_BYTES) // capi.SCAN_RAY_BYTES
    with pytest.raises(RuntimeError):
        bat.scan_occupancy([0, 1], [s, s], [ends[:n2], ends[:1]], [hits[:n2], hits[:1]])
    bat.scan_occupancy([0, 1], [s, s], [ends[:n2 - 1], ends[:1]], [hits[:n2 - 1], hits[:1]])
    holds(bat, [(SR.apply_scan(cells, s, ends500, hits500), 128, R, profile, FREE), (SR.apply_scan(cells, s, ends500[:1], hits500[:1]), 128, R, profile, FREE)])
    bat.close()


def test_one_instances_scan_changes_no_bit_of_an_instance_on_another_map():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 5, 2   # (instance 2 alone is on map 1)
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 0], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.02, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, scans, _ = scanned_twin_maps(geos)
    snaps = []
    for scanned in (False, True):
        bat = BatchController(p, B, min_shift=True)
        bat.set_occupancy(occ, INFLATION, map_of, w)
        if scanned:   # (everything in reach of the sensor becomes occupied or free)
            g = geos[1]
            ends, hits = SR.fan(scans[1][0], 720, 0.6 * max(g.nx, g.ny), hit_every=1)
            bat.scan_occupancy([1], [scans[1][0]], [ends], [hits])
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        snaps.append(BS.snapshot(bat, u, st))
        bat.close()
    assert not np.array_equal(snaps[0][j]["c"], snaps[1][j]["c"])
    assert all(BS.same_bits(snaps[0][b], snaps[1][b]) for b in range(B) if b != j)


def test_scanning_returns_all_device_and_pinned_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)
    map_of, w = np.array([b % 2 for b in range(B)], dtype=np.int32), np.full(B, 0.01)
    big = (np.ones((700, 900), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    small = (np.ones((3, 5), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    infl = batch.inflation_profile(0.5, 0.05)
    ends, hits = SR.fan((400, 300), 360, 250.0)

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        bat = BatchController(p, B)
        bat.set_occupancy([big, small], infl, map_of, w)
        for _ in range(capi.OCC_PATCH_SLOTS + 1):
            bat.scan_occupancy([0, 1], [(400, 300), (1, 1)], [ends, ends[:3]], [hits, hits[:3]])
        bat.iterate(*inputs[:6], 0)
        bat.roll_occupancy([0], [3], [-2])
        bat.scan_occupancy([0], [(400, 300)], [ends], [hits])
        bat.set_occupancy(None)
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    # the staging ring is 4 MiB of pinned, hence resident, host memory per handle: 40 rings left behind would be 160 MiB
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)

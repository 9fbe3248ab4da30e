"""GPU tests (-m gpu) of the batch handles' device-inflated costmaps (ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue;
BatchController.set_occupancy / update_occupancy).

The checker is tests/costmap_reference.py: integers and one table lookup, so the derived float cells are held against it BIT
FOR BIT, and a handle over derived cells against a handle that was given the checker's float map through _set_grids bit for
bit in everything a tick leaves.  No test asserts a time, and none checks from the host that the enqueue call did not
synchronise (section 10k says how that is held).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import batch_support as BS
import ccv_mppi_path_tracker_amd as amd
import costmap_reference as CR
import fleet_support as FS
import grid_reference as GR
import obstacle_cases as OC
from batch_support import GRID, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import INFLATION, _rss_kb, cells_hit, derived, layer_like, occ_map, same, tick_bits

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import costmap_door_cpu as CD  # noqa: E402

pytestmark = pytest.mark.gpu
u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


# 1. full inflation ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_handle():
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    yield bat
    bat.close()


@pytest.mark.parametrize("R", CR.RADII)
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_full_inflation_equals_the_checker(small_handle, nx, ny, R):
    """every layer of the CPU test's list as one map of one call; the brute-force checker"""
    bat, profile = small_handle, CR.distinct_profile(R)
    layers = CR.layers(nx, ny)
    bat.set_occupancy([occ_map(cells, threshold) for _, cells, threshold in layers], (R, profile, CR.FREE_VALUE), [0], 1.0)
    maps = bat.get_grids()[0]
    assert len(maps) == len(layers)
    for m, (name, cells, threshold) in enumerate(layers):
        assert same(maps[m][0], CR.cost_brute(cells, threshold, R, profile, CR.FREE_VALUE)), (name, nx, ny, R)
        assert same(bat.read_occupancy(m), cells), name
        assert maps[m][3] == CR.OUTSIDE


@pytest.mark.parametrize("nx,ny,R", [(300, 210, 64), (193, 129, 17), (131, 67, 3)])
def test_full_inflation_over_several_tiles(small_handle, nx, ny, R):
    """300 x 210 at R = 64: a halo spans three tiles in both directions; sizes that are no multiple of the tile in either
    direction (one cell more than three and two tiles; 131 x 67).  The separable checker (tests/test_costmap_reference.py pins it)"""
    bat, profile = small_handle, CR.distinct_profile(R)
    rng = np.random.default_rng(nx)
    for share in (0.0005, 0.02):
        cells = np.where(rng.random((ny, nx)) < share, 200, 50).astype(np.uint8)
        cells[ny - 1, nx - 1] = 200
        bat.set_occupancy([occ_map(cells)], (R, profile, CR.FREE_VALUE), [0], 1.0)
        want = CR.cost_separable(cells, 128, R, profile, CR.FREE_VALUE)
        assert len(np.unique(want)) > min(R * R, 50) // 2
        assert same(derived(bat), want), (nx, ny, R, share)


# 2. patches -------------------------------------------------------------------------------------------------------------------
def patch_list(nx, ny, rng):
    """3 * (ring size) rectangles (x0, y0, w, h, share occupied): ones that only clear, 1 x 1, a full row, the whole map, and
    rectangles touching each edge and each corner"""
    w, h = 9, 7
    rects = [(nx // 3, ny // 3, 40, 30, 0.0),                                   # only clears, where the start is dense
             (nx // 2, ny // 2, 1, 1, 1.0), (0, ny // 2, nx, 1, 0.5),           # 1 x 1; a full row
             (0, 0, nx, ny, 0.03),                                              # the whole map
             (0, ny // 4, w, h, 0.3), (nx - w, ny // 4, w, h, 0.3), (nx // 4, 0, w, h, 0.3), (nx // 4, ny - h, w, h, 0.3),   # edges
             (0, 0, w, h, 0.3), (nx - w, 0, w, h, 0.0), (0, ny - h, w, h, 0.3), (nx - w, ny - h, w, h, 0.3)]                 # corners
    assert len(rects) == 3 * capi.OCC_PATCH_SLOTS
    return [(x0, y0, np.where(rng.random((hh, ww)) < share, 200, 50).astype(np.uint8)) for x0, y0, ww, hh, share in rects]


@pytest.mark.parametrize("R", (0, 3, 17, 64))
def test_patches_back_to_back_equal_the_checker_from_scratch(small_handle, R):
    bat, profile = small_handle, CR.distinct_profile(R)
    nx, ny = 150, 100
    rng = np.random.default_rng(R)
    cells = np.where(rng.random((ny, nx)) < 0.03, 200, 50).astype(np.uint8)
    bat.set_occupancy([occ_map(cells)], (R, profile, CR.FREE_VALUE), [0], 1.0)
    for x0, y0, patch in patch_list(nx, ny, rng):
        cells = CR.apply_patch(cells, x0, y0, patch)
        buf = patch.copy()
        bat.update_occupancy(0, x0, y0, buf)    # (no synchronisation between the calls)
        buf[...] = 255 - buf                    # the caller's buffer is free as soon as the call returns
    assert same(bat.read_occupancy(0), cells)
    assert same(derived(bat), CR.cost_separable(cells, 128, R, profile, CR.FREE_VALUE))


def test_a_clearing_patch_needs_both_margins(small_handle):
    """tests/test_costmap_reference.py's case: A is cleared, B stays 2R to its right"""
    bat, R = small_handle, 17
    profile = CR.distinct_profile(R)
    cells = np.zeros((45, 67), dtype=np.uint8)
    cells[20, 20] = cells[20, 20 + 2 * R] = 1
    bat.set_occupancy([occ_map(cells, threshold=1)], (R, profile, CR.FREE_VALUE), [0], 1.0)
    bat.update_occupancy(0, 20, 20, np.zeros((1, 1), dtype=np.uint8))
    got = derived(bat)
    assert got[20, 20 + R] == profile[R * R] and got[20, 20 - R] == np.float32(CR.FREE_VALUE)
    assert same(got, CR.cost_separable(CR.apply_patch(cells, 20, 20, np.zeros((1, 1), dtype=np.uint8)), 1, R, profile, CR.FREE_VALUE))


# 3. same bits as a caller-made map ----------------------------------------------------------------------------------------------
def twin_maps(geos, seed=0):
    """(the arguments of set_occupancy's maps, the checker's float maps as set_grids takes them)"""
    R, profile, free = INFLATION
    occ, flt = [], []
    for m, g in enumerate(geos):
        cells = layer_like(g, seed + m)
        occ.append((cells, (g.ox, g.oy), g.resolution, float(g.outside), 128))
        flt.append((CR.cost_separable(cells, 128, R, profile, free), (g.ox, g.oy), g.resolution, float(g.outside)))
    return occ, flt


@pytest.mark.parametrize("discs", ["none", "static", "moving"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_derived_cells_give_the_bits_of_a_caller_made_map(shift, discs):
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, flt = twin_maps(geos)
    d = OC.discs_for(p, inputs, ns=(32, 0, 3, 3, 32)) if discs != "none" else None
    vels = [np.stack([0.3 * np.cos(np.arange(len(a)) + b), 0.2 * np.sin(np.arange(len(a)) - b)], axis=1).reshape(-1, 2)
            for b, a in enumerate(d)] if discs == "moving" else None
    s0, rseeds = BS.start_poses(p, B)
    rgeos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    rocc, rflt = twin_maps(rgeos, seed=7)
    out = []
    for source in ("occupancy", "grids"):
        bat = BatchController(p, B, min_shift=shift)
        if d is not None:
            bat.set_obstacles(d, OC.W_OBS, velocities=vels)
        if source == "occupancy":
            bat.set_occupancy(occ, INFLATION, map_of, w)
        else:
            bat.set_grids(flt, map_of, w)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res = [BS.snapshot(bat, u, st), bat.last_kernel(), derived(bat, 0), derived(bat, 1)]
        # five resident ticks over maps placed from the start poses
        if source == "occupancy":
            bat.set_occupancy(rocc, INFLATION, map_of, w)
        else:
            bat.set_grids(rflt, map_of, w)
        bat.resident_set_paths([BS.path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, rseeds)
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(tick_bits(bat) + [bat.resident_read()[0].tobytes()])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    a, b = out
    assert a[1] == b[1] == a[-1] == b[-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    assert same(a[2], b[2]) and same(a[3], b[3]) and len(np.unique(a[2])) > 5
    assert all(BS.same_bits(x, y) for x, y in zip(a[0], b[0]))
    for it in range(5):
        assert a[4 + it] == b[4 + it], it


def test_derived_cells_give_the_bits_of_a_caller_made_map_beside_the_fleet_term():
    p = FS.params("diff_drive", 1000, 15)
    B = 5
    s0, seeds, paths = FS.fleet_start(p, B)
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    occ, flt = twin_maps(geos, seed=3)
    static = [FS.far_discs(b % 3, b) for b in range(B)]
    out = []
    for source in ("occupancy", "grids"):
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0)))
        bat.resident_set_fleet_prediction(True)
        if source == "occupancy":
            bat.set_occupancy(occ, INFLATION, map_of, w)
        else:
            bat.set_grids(flt, map_of, w)
        res = []
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(tick_bits(bat) + [bat.resident_read()[0].tobytes()])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    assert out[0] == out[1] and out[0][-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT


# 4. stream order ----------------------------------------------------------------------------------------------------------------
T_STREAM = 30


@pytest.mark.parametrize("mode", ["resident", "iterate"])
def test_patches_take_effect_in_stream_order(mode):
    """A: occupancy, one patch enqueued after every step and nothing else between the steps.  B: before every step the
    checker's full map of that moment through _set_grids.  B runs first, tick by tick; patch t is placed on a cell that a state
    of its tick t read, and at least a third of the patches must change the cost of a cell that some covered state of tick
    t + 1 reads (on B's read-back candidates; A's are the same bits).  Every third patch clears a wide rectangle."""
    p = configs.diff_drive_defaults(128, 15)
    B, R = 2, 3
    profile, free = CR.distinct_profile(R) * np.float32(0.001), 0.0   # (1.000 .. 1.009: the ring costs about what a cell does)
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    geo = GR.map_ahead(s0[0, :3], p.v_ref, p.dt, p.horizon, ahead=3.0)
    map_of, w = np.array([0, -1], dtype=np.int32), np.array([0.5, 0.0])
    x0 = np.zeros((B, 3))
    x0[:, :3] = s0[:, :3]
    xr, yr, yaw0 = np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B)
    for b in range(B):
        _, xr[b], yr[b], yaw = amd.calc_ref_path(paths[b][0], paths[b][1], s0[b, 0], s0[b, 1], p.v_ref, p.dt, p.resolution, p.horizon)
        yaw0[b] = yaw[0]

    def prepare(bat):
        if mode == "resident":
            bat.resident_set_paths(paths)
            bat.resident_set_poses(s0, seeds)

    def step(bat, it):
        if mode == "resident":
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        else:
            bat.iterate_enqueue(x0, p.dt, xr, yr, yaw0, seeds, it)

    def result(bat):
        out = [bat.get_nominal().tobytes(), bat.read_costs(0).tobytes(), bat.read_costs(1).tobytes()]
        if mode == "resident":
            out += [bat.resident_read()[0].tobytes(), bat.resident_read_trace(0).tobytes(), bat.resident_read_trace(1).tobytes()]
        return out

    # B: the reference handle, which also places the patches
    cells = np.zeros((geo.ny, geo.nx), dtype=np.uint8)
    cost = CR.cost_separable(cells, 128, R, profile, free)
    ref = BatchController(p, B, min_shift=True)
    prepare(ref)
    patches, changed, looked_at = [], None, 0
    for it in range(T_STREAM):
        ref.set_grids([(cost, (geo.ox, geo.oy), geo.resolution, float(geo.outside))], map_of, w)
        step(ref, it)
        hit = cells_hit(geo, ref.read_candidates(0)[:, :GR.n_covered(p.model, p.horizon)])
        if changed is not None:
            looked_at += bool(np.intersect1d(hit, changed).size)
        assert hit.size > 0, "the fan left the map"
        if it % 3 == 2:   # clear a wide rectangle around the cells read
            iy, ix = np.divmod(hit, geo.nx)
            ax, ay = max(int(ix.min()) - 4, 0), max(int(iy.min()) - 4, 0)
            patch = (ax, ay, np.zeros((min(int(iy.max()) + 5, geo.ny) - ay, min(int(ix.max()) + 5, geo.nx) - ax), dtype=np.uint8))
        else:             # occupy a cell that a late state read
            iy, ix = divmod(int(hit[(7 * it + 3) % hit.size]), geo.nx)
            patch = (ix, iy, np.full((1, 1), 255, dtype=np.uint8))
        patches.append(patch)
        cells = CR.apply_patch(cells, *patch)
        new = CR.cost_separable(cells, 128, R, profile, free)
        changed = np.flatnonzero(new.reshape(-1) != cost.reshape(-1))
        cost = new
    want, k_ref = result(ref), ref.last_kernel()
    ref.close()
    print("[stream order, %s] %d of %d patches changed a cell that the next tick read" % (mode, looked_at, T_STREAM - 1))
    assert 3 * looked_at >= T_STREAM
    # A: occupancy, patched in stream order
    bat = BatchController(p, B, min_shift=True)
    prepare(bat)
    bat.set_occupancy([(np.zeros((geo.ny, geo.nx), dtype=np.uint8), (geo.ox, geo.oy), geo.resolution, float(geo.outside), 128)],
                      (R, profile, free), map_of, w)
    for it in range(T_STREAM):
        step(bat, it)
        bat.update_occupancy(0, *patches[it])
    got = result(bat)
    assert bat.last_kernel() == k_ref == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    assert same(bat.read_occupancy(0), cells) and same(derived(bat), cost)
    bat.close()
    assert got == want


# 5. a door closes ---------------------------------------------------------------------------------------------------------------
def test_a_door_closes():
    """tools/costmap_door_cpu.py's scenario (tests/test_costmap_door_cpu.py): a bare block patched across a straight path while the
    robot is still out of the horizon's reach.  Without the patch some trace poses lie in the cells the patch would occupy; with
    it none do."""
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    x0, y0, patch = CD.block_patch()
    inside = []
    for patched in (False, True):
        bat = BatchController(p, 1, min_shift=True)
        bat.set_occupancy([(CD.empty_layer(), CD.ORIGIN, CD.RESOLUTION, 0.0, CD.THRESHOLD)], CD.inflation(), [0], CD.WEIGHT)
        bat.resident_set_paths([CD.GW.path()])
        bat.resident_set_poses(np.array([CD.START]), np.array([CD.SEED], dtype=np.uint64))
        for it in range(CD.TICKS):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if patched and it == CD.PATCH_TICK:
                bat.update_occupancy(0, x0, y0, patch)
        trace = bat.resident_read_trace(0)[:, :2]
        assert len(trace) == CD.TICKS and bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
        inside.append(CD.in_block(trace))
        print("%s: %d poses in the block's cells, closest %.3f m, end x %.2f" % ("patched" if patched else "no patch", inside[-1],
                                                                                CD.clearance(trace), trace[-1, 0]))
        bat.close()
    assert inside[0] > 0
    assert inside[1] == 0


# 6. plumbing --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_the_setters_keep_the_layers():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, _ = twin_maps(geos)
    R, profile, free = INFLATION
    bat = BatchController(p, B)
    lib, ip = bat.lib, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    one = np.ones((1, 1), dtype=np.uint8)
    # nothing set: STATE
    assert bat.get_occupancy() == []
    assert lib.ccv_mppi_batch_update_occupancy_enqueue(bat._h, 0, 0, 0, 1, 1, one.ctypes.data_as(u8p)) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_read_occupancy(bat._h, 0, one.ctypes.data_as(u8p)) == capi.ERR_STATE
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    before, k_before = BS.snapshot(bat, u, st, states=False), bat.last_kernel()
    bat.set_occupancy(occ, INFLATION, map_of, w)

    def holds():
        got = bat.get_occupancy()
        assert len(got) == 2
        for (origin, res, outside, nx, ny, threshold, radius, free_value), (cells, o, r, out, th) in zip(got, occ):
            assert (origin, res, outside, nx, ny, threshold, radius, free_value) == (o, r, out, cells.shape[1], cells.shape[0], th, R, np.float32(free))
        for m in range(2):
            assert same(bat.read_occupancy(m), occ[m][0])
            assert same(derived(bat, m), CR.cost_separable(occ[m][0], 128, R, profile, free))
        _, mo, wt = bat.get_grids()
        assert np.array_equal(mo, map_of) and np.array_equal(wt, w)

    def tick():
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        return BS.snapshot(bat, u, st, states=False)

    holds()
    want = tick()
    assert not np.array_equal(want[1]["c"], before[1]["c"])

    def rows_of(**bad):
        cells, prof = np.ones((3, 4), dtype=np.uint8), np.ones(5, dtype=np.float32)
        prof[bad.pop("entry_at", 0)] = bad.pop("entry", 1.0)
        keep.extend([cells, prof])
        f = dict(origin_x=0.0, origin_y=0.0, resolution=0.1, outside=-1.0, nx=4, ny=3, threshold=1, cells=cells.ctypes.data_as(u8p), radius=2,
                 free_value=0.0, profile=prof.ctypes.data_as(C.POINTER(C.c_float)))
        f.update(bad)
        return ((capi.Occupancy * 1)(capi.Occupancy(f["origin_x"], f["origin_y"], f["resolution"], f["outside"], f["nx"], f["ny"], f["threshold"], f["cells"])),
                (capi.Inflation * 1)(capi.Inflation(f["radius"], f["free_value"], f["profile"])))

    def refused(rows, n, mo, wt):
        mo, wt = np.ascontiguousarray(mo, dtype=np.int32), np.ascontiguousarray(wt, dtype=np.float64)
        assert lib.ccv_mppi_batch_set_occupancy(bat._h, rows[0], rows[1], n, ip(mo), capi.dptr(wt)) == capi.ERR_INVALID_ARG

    keep, ok_mo, ok_w = [], np.zeros(B, dtype=np.int32), np.ones(B)
    refused(rows_of(cells=u8p()), 1, ok_mo, ok_w)
    refused(rows_of(profile=C.POINTER(C.c_float)()), 1, ok_mo, ok_w)
    for nx, ny in ((0, 3), (4, 0), (-1, 3), (32769, 1), (16384, 8192)):
        refused(rows_of(nx=nx, ny=ny), 1, ok_mo, ok_w)
    for res in (0.0, -0.1, np.nan, np.inf):
        refused(rows_of(resolution=res), 1, ok_mo, ok_w)
    for field in ("origin_x", "origin_y", "outside", "free_value"):
        for v in (np.nan, np.inf, -np.inf):
            refused(rows_of(**{field: v}), 1, ok_mo, ok_w)
    for v in (np.nan, np.inf):
        refused(rows_of(entry=v, entry_at=4), 1, ok_mo, ok_w)     # a non-finite profile entry, the last one
    for threshold in (-1, 256):
        refused(rows_of(threshold=threshold), 1, ok_mo, ok_w)
    for radius in (-1, capi.INFLATE_MAX_RADIUS + 1):
        refused(rows_of(radius=radius), 1, ok_mo, ok_w)
    for bad_w in (-1.0, np.nan, np.inf):
        refused(rows_of(), 1, ok_mo, [1.0, bad_w, 1.0, 1.0, 1.0])
    for bad_m in (-2, 1, 7):
        refused(rows_of(), 1, [0, 0, bad_m, 0, 0], ok_w)
    refused(rows_of(), -1, ok_mo, ok_w)
    rows = rows_of()
    assert lib.ccv_mppi_batch_set_occupancy(bat._h, rows[0], None, 1, ip(ok_mo), capi.dptr(ok_w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_occupancy(bat._h, rows[0], rows[1], 1, None, capi.dptr(ok_w)) == capi.ERR_INVALID_ARG
    # patches
    nx, ny = occ[0][0].shape[1], occ[0][0].shape[0]
    big = np.ones(capi.OCC_PATCH_MAX_CELLS + 1, dtype=np.uint8)
    for m, px, py, pw, ph in ((2, 0, 0, 1, 1), (-1, 0, 0, 1, 1), (0, -1, 0, 1, 1), (0, 0, -1, 1, 1), (0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (0, 0, 0, -1, 1),
                              (0, nx, 0, 1, 1), (0, 0, ny, 1, 1), (0, nx - 1, 0, 2, 1), (0, 0, ny - 1, 1, 2), (0, 1, 0, 2 ** 31 - 1, 1)):
        assert lib.ccv_mppi_batch_update_occupancy_enqueue(bat._h, m, px, py, pw, ph, big.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG, (m, px, py, pw, ph)
    assert lib.ccv_mppi_batch_update_occupancy_enqueue(bat._h, 0, 0, 0, 1, 1, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_occupancy(bat._h, 2, one.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_occupancy(bat._h, rows[0], rows[1], 1, None) == capi.ERR_INVALID_ARG   # two maps, room for one
    holds()
    assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, tick()))
    # the other setters keep the layers
    discs = OC.discs_for(p, inputs, ns=(0, 3, 0, 3, 0))
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_obstacles(discs, OC.W_OBS, velocities=[np.zeros((len(a), 2)) for a in discs])
    bat.set_obstacle_velocities(None)
    bat.set_obstacles(None)
    bat.set_min_shift(True)
    bat.set_min_shift(False)
    bat.resident_set_fleet(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0))
    bat.resident_set_fleet_prediction(True)
    bat.resident_set_fleet(None)
    holds()
    assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, tick()))
    # _set_occupancy(NULL) restores the kernel and the bits that ran before, twice over
    for again in range(2):
        bat.set_occupancy(None)
        assert bat.get_occupancy() == [] and bat.get_grids()[0] == []
        assert lib.ccv_mppi_batch_read_occupancy(bat._h, 0, one.ctypes.data_as(u8p)) == capi.ERR_STATE
        back = tick()
        assert bat.last_kernel() == k_before and all(BS.same_bits(a, b, states=False) for a, b in zip(before, back))
        bat.set_occupancy(occ, INFLATION, map_of, w)
        assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, tick()))
    # _set_grids drops the layers: the maps are the caller's
    bat.set_grids([(derived(bat, 0), occ[0][1], occ[0][2], occ[0][3]), (derived(bat, 1), occ[1][1], occ[1][2], occ[1][3])], map_of, w)
    assert bat.get_occupancy() == []
    assert lib.ccv_mppi_batch_read_occupancy(bat._h, 0, one.ctypes.data_as(u8p)) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_update_occupancy_enqueue(bat._h, 0, 0, 0, 1, 1, one.ctypes.data_as(u8p)) == capi.ERR_STATE
    assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, tick()))
    bat.close()


def test_the_patch_size_limit():
    """a patch of exactly CCV_MPPI_OCC_PATCH_MAX_CELLS cells fills a staging slot and is taken; one row more is refused"""
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    nx, ny = 1024, 1026
    assert nx * 1024 == capi.OCC_PATCH_MAX_CELLS
    cells = np.zeros((ny, nx), dtype=np.uint8)
    bat.set_occupancy([occ_map(cells, threshold=1)], (0, np.ones(1, dtype=np.float32), 0.0), [0], 1.0)
    rng = np.random.default_rng(5)
    patch = (rng.random((1025, nx)) < 0.5).astype(np.uint8)
    assert bat.lib.ccv_mppi_batch_update_occupancy_enqueue(bat._h, 0, 0, 1, nx, 1025, patch.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert not bat.read_occupancy(0).any()
    bat.update_occupancy(0, 0, 1, patch[:1024])
    cells[1:1025] = patch[:1024]
    assert same(bat.read_occupancy(0), cells) and same(derived(bat), cells.astype(np.float32))
    bat.close()


def test_one_instances_map_or_patch_changes_no_bit_of_an_instance_on_another_map():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 5, 2   # (instance 2 is on map 1, with instance 4)
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 0], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.02, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, _ = twin_maps(geos)
    other = (255 - occ[1][0],) + occ[1][1:]
    snaps = []
    for variant in ("base", "map", "patch"):
        bat = BatchController(p, B, min_shift=True)
        bat.set_occupancy([occ[0], other if variant == "map" else occ[1]], INFLATION, map_of, w)
        if variant == "patch":
            bat.update_occupancy(1, 0, 0, np.full(occ[1][0].shape, 255, dtype=np.uint8))
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        snaps.append(BS.snapshot(bat, u, st))
        bat.close()
    for s in snaps[1:]:
        assert not np.array_equal(snaps[0][j]["c"], s[j]["c"])
        assert all(BS.same_bits(snaps[0][b], s[b]) for b in range(B) if b != j)


def test_costmap_returns_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)
    map_of, w = np.array([b % 2 for b in range(B)], dtype=np.int32), np.full(B, 0.01)
    big = (np.ones((700, 900), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)      # (0.6 MiB of layer, 2.4 MiB of cells)
    small = (np.ones((3, 5), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    infl = batch.inflation_profile(0.5, 0.05)
    patch = np.zeros((64, 64), dtype=np.uint8)

    def cycle():
        bat = BatchController(p, B)
        bat.set_occupancy([big, small], infl, map_of, w)
        bat.set_occupancy([small, big], infl, map_of, w)   # (a new set is a new allocation: the old one must go)
        for _ in range(capi.OCC_PATCH_SLOTS + 1):
            bat.update_occupancy(1, 10, 10, patch)
        bat.iterate(*inputs[:6], 0)
        bat.set_grids([(np.ones((3, 5), dtype=np.float32), (0.0, 0.0), 0.05, 0.0)], np.zeros(B, dtype=np.int32), w)   # (drops the layers)
        bat.set_occupancy([big], infl, np.zeros(B, dtype=np.int32), w)
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    rss0 = _rss_kb()
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    rss1 = _rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    # the staging ring is 4 MiB of pinned, hence resident, host memory per handle: 40 rings left behind would be 160 MiB
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)


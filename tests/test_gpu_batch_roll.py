"""GPU tests (-m gpu) of the batch handles' rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue; BatchController.roll_occupancy;
DESIGN.md section 10m).

The contract is one sentence: after a roll the float cells, the layer and the origin of a map are, in every bit, what a fresh
_set_occupancy of the rolled layer at the rolled origin would produce.  The checker is tests/roll_reference.py on top of
tests/costmap_reference.py -- integers, one table lookup, one product and one sum per origin -- so everything is held against it
with no tolerance, and a rolled handle against a twin that was given the checker's float map through _set_grids bit for bit in
everything a tick leaves.  No test asserts a time, and none checks from the host that the call did not synchronise.
"""
import ctypes as C

import numpy as np
import pytest

import batch_support as BS
import costmap_reference as CR
import costmap_support as CS
import fleet_support as FS
import grid_reference as GR
import obstacle_cases as OC
import roll_reference as RR
from batch_support import GRID, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import derived, occ_map, same

pytestmark = pytest.mark.gpu
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
ORIGIN0, RES = (-1.7, 0.3), 0.05
FREE = CR.FREE_VALUE


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.fixture(scope="module")
def small_handle():
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    yield bat
    bat.close()


def window(nx, ny, seed, share=0.1):
    """a caller's new window: occupied and free under the thresholds 100 and 128 of the layers"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((ny, nx)) < share, 200, 50).astype(np.uint8)


def holds(bat, want):
    """want: per map (layer, origin, threshold, R, profile, free_value), or None for a map not to look at"""
    grids, occ = bat.get_grids()[0], bat.get_occupancy()
    assert len(grids) == len(occ) == len(want)
    for m, w in enumerate(want):
        if w is None:
            continue
        cells, origin, threshold, R, profile, free = w
        assert same(bat.read_occupancy(m), cells), m
        assert same(grids[m][0], CR.cost_separable(cells, threshold, R, profile, free)), m
        assert grids[m][1] == origin and occ[m][0] == origin, (m, grids[m][1], occ[m][0], origin)
        assert occ[m][3:5] == (cells.shape[1], cells.shape[0]) and occ[m][5:7] == (threshold, R)


# 1. one roll against the checker ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", CR.RADII)
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_one_roll_equals_the_checker_from_scratch(small_handle, nx, ny, R):
    """every layer of the CPU list as one map, all rolled by one call, per shift of the CPU list; odd maps from strips, even ones
    from fill"""
    bat, profile = small_handle, CR.distinct_profile(R)
    layers = RR.layers(nx, ny)
    for k, (dx, dy) in enumerate(RR.shifts(nx, ny)):
        bat.set_occupancy([occ_map(cells, threshold, ORIGIN0, RES) for _, cells, threshold in layers], (R, profile, FREE), [0], 1.0)
        fill, exposed, want = (255 if k % 2 else 0), [], []
        for m, (_, cells, threshold) in enumerate(layers):
            strips = RR.strips_of(window(nx, ny, 31 * k + m), dx, dy) if (m + k) % 2 else None
            exposed.append(strips)
            want.append((RR.roll_layer(cells, dx, dy, strips=strips, fill=fill), RR.rolled_origin(ORIGIN0, (dx, dy), RES), threshold, R, profile,
                         FREE))
        bat.roll_occupancy(np.arange(len(layers)), dx, dy, exposed, fill=fill)
        holds(bat, want)


def test_bands_wider_than_a_tile_across_tiles(small_handle):
    """193 x 129 at R = 64 rolled by (-70, 64): the leading bands are 134 and 128 cells wide, the map three and two tiles and a
    cell more"""
    bat, R, (nx, ny), (dx, dy) = small_handle, 64, (193, 129), (-70, 64)
    profile = CR.distinct_profile(R)
    for share in (0.0005, 0.02):
        cells = window(nx, ny, 7, share)
        cells[0, 0] = cells[ny - 1, nx - 1] = 200
        strips = RR.strips_of(window(nx, ny, 8, share), dx, dy)
        bat.set_occupancy([occ_map(cells, 128, ORIGIN0, RES)], (R, profile, FREE), [0], 1.0)
        bat.roll_occupancy([0], [dx], [dy], [strips])
        new = RR.roll_layer(cells, dx, dy, strips=strips)
        assert len(np.unique(CR.cost_separable(new, 128, R, profile, FREE))) > 25
        holds(bat, [(new, RR.rolled_origin(ORIGIN0, (dx, dy), RES), 128, R, profile, FREE)])


# 2. many maps in one call -------------------------------------------------------------------------------------------------------
def test_many_maps_of_different_sizes_in_one_call(small_handle):
    bat = small_handle
    sizes = [(67, 45), (130, 70), (1, 200), (200, 1), (33, 91), (40, 30)]
    radii = [3, 17, 64, 1, 0, 5]
    moves = {0: (3, -2), 1: (0, 0), 2: (0, 9), 3: (-205, 0), 4: (-1, 7)}   # map 1 stays, map 3 is all new, map 5 is not named
    layers = [window(nx, ny, 50 + m, 0.04) for m, (nx, ny) in enumerate(sizes)]
    infl = [(R, CR.distinct_profile(R) + np.float32(m), FREE - m) for m, R in enumerate(radii)]
    origins = [(0.25 * m, -1.0 - m) for m in range(6)]
    bat.set_occupancy([occ_map(cells, 128, origins[m], RES) for m, cells in enumerate(layers)], infl, [0], 1.0)
    before5 = (bat.read_occupancy(5), derived(bat, 5))
    order = [4, 0, 2, 1, 3]
    exposed = {m: (RR.strips_of(window(*sizes[m], 60 + m, 0.3), *moves[m]) if m in (0, 3, 4) else None) for m in order}
    bat.roll_occupancy(order, [moves[m][0] for m in order], [moves[m][1] for m in order], [exposed[m] for m in order], fill=255)
    want = []
    for m in range(5):
        new = RR.roll_layer(layers[m], *moves[m], strips=exposed[m], fill=255)
        want.append((new, RR.rolled_origin(origins[m], moves[m], RES), 128) + infl[m])
    assert same(want[1][0], layers[1]) and want[1][1] == origins[1]
    holds(bat, want + [(layers[5], origins[5], 128) + infl[5]])
    assert same(bat.read_occupancy(5), before5[0]) and same(derived(bat, 5), before5[1])


# 3. back to back ----------------------------------------------------------------------------------------------------------------
def raw_roll(bat, maps, dx, dy, buf, fill=0):
    """the C call over the caller's own arrays, which are overwritten as soon as it returns"""
    maps, dx, dy = (np.array(a, dtype=np.int32) for a in (maps, dx, dy))
    rc = bat.lib.ccv_mppi_batch_roll_occupancy_enqueue(bat._h, len(maps), maps.ctypes.data_as(i32p), dx.ctypes.data_as(i32p), dy.ctypes.data_as(i32p),
                                                       buf.ctypes.data_as(u8p) if buf is not None else None, fill)
    assert rc == capi.OK, bat.lib.ccv_mppi_batch_last_error(bat._h)
    maps[...] = -5
    dx[...] = 12345
    dy[...] = -12345
    if buf is not None:
        buf[...] = 255 - buf


@pytest.mark.parametrize("n_rolls", (12, 13))
def test_rolls_and_patches_back_to_back(small_handle, n_rolls):
    """n_rolls roll calls (map 0 in every one, and one of them moves nothing: 11 and 12 buffer swaps, an odd and an even number;
    map 1 in every third) and as many patches, interleaved with no synchronisation: 2 * n_rolls calls through a ring of
    CCV_MPPI_OCC_PATCH_SLOTS slots.  Everything is read once, at the end."""
    bat = small_handle
    sizes, radii = [(150, 100), (67, 45)], [17, 3]
    rng = np.random.default_rng(n_rolls)
    cells = [window(nx, ny, 70 + m, 0.03) for m, (nx, ny) in enumerate(sizes)]
    infl = [(R, CR.distinct_profile(R), FREE) for R in radii]
    bat.set_occupancy([occ_map(c, 128, ORIGIN0, RES) for c in cells], infl, [0], 1.0)
    raw_roll(bat, [0, 1], [0, 0], [0, 0], None)   # the priming call
    c = [[0, 0], [0, 0]]
    assert 2 * n_rolls > capi.OCC_PATCH_SLOTS
    for i in range(n_rolls):
        maps = [1, 0] if i % 3 == 0 else [0]
        moves = [(int(rng.integers(-20, 21)), int(rng.integers(-20, 21))) for _ in maps]
        if i == 5:
            moves[-1] = (0, 0)   # a call that moves nothing takes no slot
        entries = []
        for m, (dx, dy) in zip(maps, moves):
            strips = RR.strips_of(window(*sizes[m], 1000 + 10 * i + m, 0.05), dx, dy)
            entries.append(strips)
            cells[m] = RR.roll_layer(cells[m], dx, dy, strips=strips)
            c[m] = [c[m][0] + dx, c[m][1] + dy]
        raw_roll(bat, maps, [d[0] for d in moves], [d[1] for d in moves], RR.pack_strips(entries))
        m = i % 2
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        x0, y0 = int(rng.integers(0, sizes[m][0] - w + 1)), int(rng.integers(0, sizes[m][1] - h + 1))
        patch = np.where(rng.random((h, w)) < (0.0 if i % 4 == 1 else 0.3), 200, 50).astype(np.uint8)
        cells[m] = CR.apply_patch(cells[m], x0, y0, patch)
        buf = patch.copy()
        bat.update_occupancy(m, x0, y0, buf)
        buf[...] = 255 - buf
    holds(bat, [(cells[m], RR.rolled_origin(ORIGIN0, c[m], RES), 128) + infl[m] for m in range(2)])


# 4. the same bits as a twin -----------------------------------------------------------------------------------------------------
INFLATION = CS.INFLATION


def rolled_twin_maps(geos, moves, seed=0):
    """(set_occupancy's maps before the roll, the strips, the checker's float maps after it as set_grids takes them)"""
    R, profile, free = INFLATION
    occ, exposed, flt = [], [], []
    for m, (g, (dx, dy)) in enumerate(zip(geos, moves)):
        origin0 = (g.ox - dx * g.resolution, g.oy - dy * g.resolution)   # (so that the rolled window lies about where g does)
        cells = CS.layer_like(g, seed + m)
        strips = RR.strips_of(CS.layer_like(g, seed + 10 + m), dx, dy)
        new = RR.roll_layer(cells, dx, dy, strips=strips)
        occ.append((cells, origin0, g.resolution, float(g.outside), 128))
        exposed.append(strips)
        flt.append((CR.cost_separable(new, 128, R, profile, free), RR.rolled_origin(origin0, (dx, dy), g.resolution), g.resolution, float(g.outside)))
    return occ, exposed, flt


MOVES = [(3, -2), (-5, 1)]


@pytest.mark.parametrize("discs", ["none", "static", "moving"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_a_rolled_handle_gives_the_bits_of_a_twin(shift, discs):
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, exposed, flt = rolled_twin_maps(geos, MOVES)
    d = OC.discs_for(p, inputs, ns=(32, 0, 3, 3, 32)) if discs != "none" else None
    vels = [np.stack([0.3 * np.cos(np.arange(len(a)) + b), 0.2 * np.sin(np.arange(len(a)) - b)], axis=1).reshape(-1, 2)
            for b, a in enumerate(d)] if discs == "moving" else None
    s0, rseeds = BS.start_poses(p, B)
    rgeos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    rocc, rexposed, rflt = rolled_twin_maps(rgeos, MOVES[::-1], seed=7)
    out = []
    for source in ("rolled", "grids"):
        bat = BatchController(p, B, min_shift=shift)
        if d is not None:
            bat.set_obstacles(d, OC.W_OBS, velocities=vels)
        if source == "rolled":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            bat.set_nominal(nom)
            bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)   # (a tick over the maps before the roll)
            k0 = bat.last_kernel()
            bat.roll_occupancy([0, 1], [m[0] for m in MOVES], [m[1] for m in MOVES], exposed)
            assert bat.last_kernel() == k0
        else:
            bat.set_grids(flt, map_of, w)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res = [BS.snapshot(bat, u, st), bat.last_kernel(), derived(bat, 0), derived(bat, 1)]
        # five resident ticks over maps placed from the start poses
        if source == "rolled":
            bat.set_occupancy(rocc, INFLATION, map_of, w)
            bat.roll_occupancy([1, 0], [m[0] for m in MOVES], [m[1] for m in MOVES], rexposed[::-1])
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


def test_a_rolled_handle_gives_the_bits_of_a_twin_beside_the_fleet_term():
    p = FS.params("diff_drive", 1000, 15)
    B = 5
    s0, seeds, paths = FS.fleet_start(p, B)
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    occ, exposed, flt = rolled_twin_maps(geos, MOVES, seed=3)
    static = [FS.far_discs(b % 3, b) for b in range(B)]
    out = []
    for source in ("rolled", "grids"):
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0)))
        bat.resident_set_fleet_prediction(True)
        if source == "rolled":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            bat.roll_occupancy([0, 1], [m[0] for m in MOVES], [m[1] for m in MOVES], exposed)
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


def world(c, nx, ny):
    """the occupancy of the world's cells under a window of nx x ny cells whose corner cell is c: a fixed pseudo-random field,
    about 6 % occupied"""
    gx = (int(c[0]) + np.arange(nx, dtype=np.int64))[None, :]
    gy = (int(c[1]) + np.arange(ny, dtype=np.int64))[:, None]
    h = ((gx * 73856093) ^ (gy * 19349663)) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 0x5BD1E995) & 0xFFFFFFFF
    return np.where((h >> 8) % 100 < 6, 255, 0).astype(np.uint8)


def test_rolls_take_effect_in_stream_order():
    """A: occupancy, one roll with strips enqueued after every resident step and nothing else between the steps.  B: before every
    step the checker's full map of that moment, at the rolled origin, through _set_grids.  B runs first, tick by tick, and
    decides the rolls: the window, which ends about half the fan's reach ahead, follows instance 0's pose by whole cells.  At
    least a third of the rolls must change what a covered state of the next tick reads (on B's read-back candidates; A's are the
    same bits): a state that read `outside`, or a cell near the edge, reads another value under the rolled map."""
    p = configs.diff_drive_defaults(128, 15)
    B, R = 2, 3
    profile, free = CR.distinct_profile(R) * np.float32(0.001), 0.0
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    geo = GR.map_ahead(s0[0, :3], p.v_ref, p.dt, p.horizon, ahead=0.5)
    nx, ny, res, origin0, outside = geo.nx, geo.ny, geo.resolution, (geo.ox, geo.oy), 0.5
    map_of, w = np.array([0, -1], dtype=np.int32), np.array([0.5, 0.0])
    ncov = GR.n_covered(p.model, p.horizon)

    def grid_at(c):
        return GR.Grid(CR.cost_separable(world(c, nx, ny), 128, R, profile, free), RR.rolled_origin(origin0, c, res), res, outside)

    def result(bat):
        return [bat.get_nominal().tobytes(), bat.read_costs(0).tobytes(), bat.read_costs(1).tobytes(), bat.resident_read()[0].tobytes(),
                bat.resident_read_trace(0).tobytes(), bat.resident_read_trace(1).tobytes()]

    # B: the reference handle, which also decides the rolls
    ref = BatchController(p, B, min_shift=True)
    ref.resident_set_paths(paths)
    ref.resident_set_poses(s0, seeds)
    c, rolls, mattered, prev = (0, 0), [], 0, None
    for it in range(T_STREAM):
        g = grid_at(c)
        ref.set_grids([g.as_tuple()], map_of, w)
        ref.resident_step_enqueue(p.dt, it, advance=it > 0)
        P = ref.read_candidates(0)[:, :ncov]
        if prev is not None:   # what this tick's states read under the map before the last roll and under the one after it
            mattered += not same(GR.lookup(prev, P[..., 0], P[..., 1])[0], GR.lookup(g, P[..., 0], P[..., 1])[0])
        assert GR.lookup(g, P[..., 0], P[..., 1])[1].any(), "the fan left the map"
        pose = ref.resident_read()[0][0]
        target = (int(np.floor((pose[0] - s0[0, 0]) / res)), int(np.floor((pose[1] - s0[0, 1]) / res)))
        rolls.append((target[0] - c[0], target[1] - c[1]))
        prev, c = g, target
    want, k_ref = result(ref), ref.last_kernel()
    ref.close()
    moved = sum(1 for d in rolls[:-1] if d != (0, 0))
    print("[stream order] %d of %d rolls changed what the next tick read (%d moved the window; it ended %s cells from its start)"
          % (mattered, T_STREAM - 1, moved, c))
    assert 3 * mattered >= T_STREAM
    # A: occupancy, rolled in stream order
    bat = BatchController(p, B, min_shift=True)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    bat.set_occupancy([(world((0, 0), nx, ny), origin0, res, outside, 128)], (R, profile, free), map_of, w)
    bat.roll_occupancy([0], [0], [0])   # the priming call: the rolls below allocate nothing
    c = (0, 0)
    for it in range(T_STREAM):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        dx, dy = rolls[it]
        c = (c[0] + dx, c[1] + dy)
        bat.roll_occupancy([0], [dx], [dy], [RR.strips_of(world(c, nx, ny), dx, dy)])
    got = result(bat)
    assert bat.last_kernel() == k_ref == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    last = grid_at(c)
    assert same(bat.read_occupancy(0), world(c, nx, ny)) and same(derived(bat), last.cells)
    assert bat.get_grids()[0][0][1] == (last.ox, last.oy)
    bat.close()
    assert got == want


# 6. plumbing --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_the_setters_keep_the_rolled_map():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    geos = [GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m) for m, b in enumerate((1, 2))]
    occ, exposed, flt = rolled_twin_maps(geos, MOVES)
    R, profile, free = INFLATION
    bat = BatchController(p, B)
    lib = bat.lib
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(i32p)   # noqa: E731
    call = lib.ccv_mppi_batch_roll_occupancy_enqueue
    # nothing set, and a caller's float maps: STATE
    assert call(bat._h, 1, ip([0]), ip([1]), ip([0]), None, 0) == capi.ERR_STATE
    bat.set_grids(flt, map_of, w)
    assert call(bat._h, 1, ip([0]), ip([1]), ip([0]), None, 0) == capi.ERR_STATE
    bat.set_occupancy(occ, INFLATION, map_of, w)

    def tick():
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        return BS.snapshot(bat, u, st, states=False)

    def state():
        return [bat.read_occupancy(m).tobytes() + derived(bat, m).tobytes() for m in range(2)] + [bat.get_occupancy(), bat.get_grids()[0][0][1]]

    # the priming roll changes no bit
    before, bits = state(), tick()
    bat.roll_occupancy([0, 1], 0, 0)
    bat.roll_occupancy([1], 0, 0, [(None, None)])
    assert state() == before and all(BS.same_bits(a, b, states=False) for a, b in zip(bits, tick()))
    # one roll, then every refusal
    bat.roll_occupancy([0, 1], [m[0] for m in MOVES], [m[1] for m in MOVES], exposed)
    rolled = [(RR.roll_layer(occ[m][0], *MOVES[m], strips=exposed[m]), RR.rolled_origin(occ[m][1], MOVES[m], occ[m][2]), 128, R, profile,
               np.float32(free)) for m in range(2)]
    holds(bat, rolled)
    before, bits = state(), tick()
    big = np.zeros(1 << 16, dtype=np.uint8)
    far = 32768 + 1   # CCV_MPPI_GRID_MAX_DIM + 1
    for n, maps, dx, dy, buf, fill in ((0, [0], [1], [0], None, 0), (3, [0, 1, 0], [1, 1, 1], [0, 0, 0], None, 0), (-1, [0], [1], [0], None, 0),
                                       (1, [2], [1], [0], None, 0), (1, [-1], [1], [0], None, 0), (2, [1, 1], [1, 1], [0, 0], None, 0),
                                       (2, [0, 0], [0, 0], [0, 0], None, 0),
                                       (1, [0], [far], [0], None, 0), (1, [0], [0], [-far], None, 0), (1, [0], [-2 ** 31], [0], None, 0),
                                       (1, [0], [1], [0], None, -1), (1, [0], [1], [0], None, 256), (1, [0], [0], [0], None, 256)):
        rc = call(bat._h, n, ip(maps), ip(dx), ip(dy), None if buf is None else buf.ctypes.data_as(u8p), fill)
        assert rc == capi.ERR_INVALID_ARG, (n, maps, dx, dy, fill)
    assert call(bat._h, 1, None, ip([1]), ip([0]), None, 0) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), None, ip([0]), None, 0) == capi.ERR_INVALID_ARG
    assert call(bat._h, 1, ip([0]), ip([1]), None, big.ctypes.data_as(u8p), 0) == capi.ERR_INVALID_ARG
    assert state() == before and all(BS.same_bits(a, b, states=False) for a, b in zip(bits, tick()))
    # the other setters keep the rolled map and its origin
    discs = OC.discs_for(p, inputs, ns=(0, 3, 0, 3, 0))
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_obstacles(discs, OC.W_OBS, velocities=[np.zeros((len(a), 2)) for a in discs])
    bat.set_obstacle_velocities(None)
    bat.set_obstacles(None)
    bat.set_min_shift(True)
    bat.set_min_shift(False)
    holds(bat, rolled)
    assert state() == before and all(BS.same_bits(a, b, states=False) for a, b in zip(bits, tick()))
    # a patch addresses the rolled frame
    patch = np.full((3, 4), 255, dtype=np.uint8)
    bat.update_occupancy(0, 2, 1, patch)
    rolled[0] = (CR.apply_patch(rolled[0][0], 2, 1, patch),) + rolled[0][1:]
    holds(bat, rolled)
    # _set_occupancy after rolls starts again from its own origin with no cell moved
    bat.set_occupancy(occ, INFLATION, map_of, w)
    holds(bat, [(occ[m][0], occ[m][1], 128, R, profile, np.float32(free)) for m in range(2)])
    bat.roll_occupancy([1], [1], [0])
    holds(bat, [None, (RR.roll_layer(occ[1][0], 1, 0), RR.rolled_origin(occ[1][1], (1, 0), occ[1][2]), 128, R, profile, np.float32(free))])
    # the float maps are a caller's again: no roll
    bat.set_grids(flt, map_of, w)
    assert call(bat._h, 1, ip([0]), ip([1]), ip([0]), None, 0) == capi.ERR_STATE
    bat.close()


def test_the_origin_is_refused_where_it_would_not_be_finite_and_the_offset_at_its_limit():
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    cells, infl = np.zeros((1, 1), dtype=np.uint8), (0, np.ones(1, dtype=np.float32), 0.0)
    bat.set_occupancy([(cells, (1.7e308, 0.0), 1e303, 0.0, 1)], infl, [0], 1.0)
    with pytest.raises(RuntimeError):
        bat.roll_occupancy([0], [32768], [0])
    bat.roll_occupancy([0], [-32768], [32768], fill=7)
    assert bat.get_occupancy()[0][0] == RR.rolled_origin((1.7e308, 0.0), (-32768, 32768), 1e303) and bat.read_occupancy(0)[0, 0] == 7
    # 2^30 cells in steps of 2^15: the last step to the limit is taken, the next one refused, the origin exact
    bat.set_occupancy([(cells, (0.1, -0.1), 0.05, 0.0, 1)], infl, [0], 1.0)
    m, dx, dy = (np.array([v], dtype=np.int32) for v in (0, 32768, -32768))
    for _ in range(32768):
        assert bat.lib.ccv_mppi_batch_roll_occupancy_enqueue(bat._h, 1, m.ctypes.data_as(i32p), dx.ctypes.data_as(i32p), dy.ctypes.data_as(i32p), None, 3) == capi.OK
    for ex, ey in ((1, 0), (0, -1)):
        with pytest.raises(RuntimeError):
            bat.roll_occupancy([0], [ex], [ey])
    assert bat.get_occupancy()[0][0] == RR.rolled_origin((0.1, -0.1), (2 ** 30, -2 ** 30), 0.05) == bat.get_grids()[0][0][1]
    assert bat.read_occupancy(0)[0, 0] == 3
    bat.roll_occupancy([0], [-1], [1])
    bat.close()


def test_the_slot_size_limit():
    """tables and strips share one staging slot: a strip of 1023 rows of 1024 cells fits beside the 336 bytes of tables, 1024 rows
    do not"""
    bat = BatchController(configs.diff_drive_defaults(128, 15), 1)
    nx, ny = 1024, 1026
    cells = np.zeros((ny, nx), dtype=np.uint8)
    bat.set_occupancy([occ_map(cells, threshold=1)], (0, np.ones(1, dtype=np.float32), 0.0), [0], 1.0)
    win = (np.random.default_rng(5).random((ny, nx)) < 0.5).astype(np.uint8)
    with pytest.raises(RuntimeError):
        bat.roll_occupancy([0], [0], [1024], [RR.strips_of(win, 0, 1024)])
    assert not bat.read_occupancy(0).any() and bat.get_occupancy()[0][0] == (0.0, 0.0)
    bat.roll_occupancy([0], [0], [1023], [RR.strips_of(win, 0, 1023)])
    new = RR.roll_layer(cells, 0, 1023, strips=RR.strips_of(win, 0, 1023))
    assert same(bat.read_occupancy(0), new) and same(derived(bat), new.astype(np.float32))
    bat.roll_occupancy([0], [0], [-2000], fill=1)   # (with fill there are no strips: any shift fits)
    assert bat.read_occupancy(0).all()
    bat.close()


def test_rolling_returns_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)
    map_of, w = np.array([b % 2 for b in range(B)], dtype=np.int32), np.full(B, 0.01)
    big = (np.ones((700, 900), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)      # (0.6 MiB of layer, 2.4 MiB of cells, twice over)
    small = (np.ones((3, 5), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    infl = batch.inflation_profile(0.5, 0.05)

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle(close=True):
        bat = BatchController(p, B)
        bat.set_occupancy([big, small], infl, map_of, w)
        bat.roll_occupancy([0, 1], [3, 1], [-2, 0])
        bat.set_occupancy([small, big], infl, map_of, w)   # (a new set: the second allocation goes with the old layers)
        for _ in range(capi.OCC_PATCH_SLOTS + 1):
            bat.roll_occupancy([1], [1], [1])
        bat.iterate(*inputs[:6], 0)
        bat.set_grids([(np.ones((3, 5), dtype=np.float32), (0.0, 0.0), 0.05, 0.0)], np.zeros(B, dtype=np.int32), w)   # (drops all four)
        bat.set_occupancy([big], infl, np.zeros(B, dtype=np.int32), w)
        bat.roll_occupancy([0], [0], [0])
        bat.set_occupancy(None)
        bat.set_occupancy([big], infl, np.zeros(B, dtype=np.int32), w)
        bat.roll_occupancy([0], [-700], [900], fill=1)
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)
    # _set_grids and _set_occupancy(NULL) give the second allocation back with the first, while the handle lives
    bat = BatchController(p, B)
    huge = (np.ones((4000, 3000), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)   # 12 MB of layer, 48 MB of cells, twice over
    for drop in (lambda: bat.set_occupancy(None), lambda: bat.set_grids([(np.ones((3, 5), dtype=np.float32), (0.0, 0.0), 0.05, 0.0)], map_of * 0, w)):
        bat.set_occupancy([small], infl, map_of * 0, w)
        base = level()
        bat.set_occupancy([huge], infl, map_of * 0, w)
        one = base - level()
        bat.roll_occupancy([0], [1], [0])
        two = base - level()
        assert one >= 50 * 2**20 and two - one >= 50 * 2**20, (one, two)
        drop()
        assert base - level() < 16 * 2**20, "%.1f MiB not returned" % ((base - level()) / 2**20)
    bat.close()

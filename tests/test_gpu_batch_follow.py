"""GPU tests (-m gpu) of the costmaps that follow their robots (ccv_mppi_batch_resident_set_follow, _follow_enqueue, _read_follow,
_plan_goals_enqueue; BatchController.resident_follow).

The reference of every assertion is a twin handle on the calls that were there before: it reads its poses back (_resident_read),
decides with the checker (tests/follow_reference.py) and rolls with _roll_occupancy_enqueue(exposed=None, fill); it senses with
_resident_sense_enqueue and plans with batch.goal_cells and _resident_plan_enqueue.  The following handle reads nothing until it
is compared.  Everything is compared bit for bit; there is no tolerance.  Most maps have a resolution of 2^-2 or 2^-4 and origins
that are multiples of it, so that a pose can be put exactly on a cell edge; one test follows at 0.05 m cells, where every step rounds.  _resident_set_poses takes a NaN pose, so the NaN
case runs on the device.  The 2^30 limit of the accumulated offset is held on the CPU only (tests/test_follow_reference.py)."""
import ctypes as C

import numpy as np
import pytest

import batch_support as BS
import costmap_reference as CR
import costmap_support as CS
import follow_reference as FR
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import derived, same

pytestmark = pytest.mark.gpu
i32p = C.POINTER(C.c_int32)
RES, ORIGIN = 0.25, (-3.0, 1.5)
FREE = CR.FREE_VALUE
P = configs.diff_drive_defaults(64, 5)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def lines(B, res=RES, n=40, origin=ORIGIN):
    return [(origin[0] + res * np.arange(float(n)), np.full(n, origin[1] + 0.5 * b)) for b in range(B)]


def make(B, res=RES):
    bat = BatchController(P, B)
    bat.resident_set_paths(lines(B, res), res)
    return bat


@pytest.fixture(scope="module")
def pair7():
    a, b = make(7), make(7)
    yield a, b
    BS.close_all(a, b)


@pytest.fixture(scope="module")
def pair3():
    a, b = make(3), make(3)
    yield a, b
    BS.close_all(a, b)


def set_poses(bats, xy):
    st = np.zeros((bats[0].B, 3))
    st[:len(xy), :2] = np.asarray(xy, dtype=np.float64)
    for bat in bats:
        bat.resident_set_poses(st, np.arange(1, bat.B + 1, dtype=np.uint64))
    return st


def layer(nx, ny, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((ny, nx)) < 0.08, 255, 0).astype(np.uint8)


class Twin:
    """the twin handle and what the checker knows of its maps: the offsets, the origins they were set with, the last rows"""

    def __init__(self, bat, origins0, res, map_of):
        self.bat, self.o0, self.res, self.map_of = bat, [tuple(o) for o in origins0], res, list(map_of)
        n = len(origins0)
        self.c = np.zeros((n, 2), dtype=np.int64)
        self.status, self.shift = np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32)

    def frame(self, m):
        geo = self.bat.get_occupancy()[m]
        return (int(self.c[m, 0]), int(self.c[m, 1]), geo[0][0], geo[0][1]), (self.o0[m], self.res, geo[3], geo[4])

    def follow(self, instances, margin, max_step, fill=0):
        st = self.bat.resident_read()[0]
        maps, dxs, dys = [], [], []
        for b in instances:
            m = self.map_of[b]
            frame, geo = self.frame(m)
            status, dx, dy, new = FR.decide(frame, st[b, :2], geo, margin, max_step)
            self.status[m], self.shift[m] = status, (dx, dy)
            if status == FR.MOVED:
                maps.append(m), dxs.append(dx), dys.append(dy)
                self.c[m] = new[:2]
        if maps:
            self.bat.roll_occupancy(maps, dxs, dys, None, fill)
        return [int(self.status[self.map_of[b]]) for b in instances]

    def holds(self, bat, rows=True):
        """the following handle `bat` equals the twin in the layers, the float cells, the origins and the rows of _read_follow"""
        want, got = self.bat.get_occupancy(), bat.get_occupancy()
        assert want == got, (want, got)
        for m in range(len(want)):
            assert same(bat.read_occupancy(m), self.bat.read_occupancy(m)), m
            assert same(derived(bat, m), derived(self.bat, m)), m
        assert [g[1] for g in bat.get_grids()[0]] == [g[1] for g in self.bat.get_grids()[0]]
        if rows:
            status, shift, offset, origin = bat.resident_read_follow()
            assert status.tolist() == self.status.tolist(), (status, self.status)
            assert shift.tolist() == self.shift.tolist(), (shift, self.shift)
            assert offset.dtype == np.int64 and offset.tolist() == self.c.tolist(), (offset, self.c)
            assert origin.tolist() == [list(g[0]) for g in want]


def same_tick(bat, twin, it):
    """one tick of both (the poses stay), and everything it leaves"""
    for h in (bat, twin):
        h.resident_step_enqueue(P.dt, it, advance=False)
    a, b = CS.tick_bits(bat), CS.tick_bits(twin)
    assert a == b, [i for i, (x, y) in enumerate(zip(a, b)) if x != y]


def install(bats, layers, R, map_of, res=RES, origins=None, weight=1.0):
    origins = origins or [(ORIGIN[0] + 2.0 * m, ORIGIN[1] - 1.0 * m) for m in range(len(layers))]
    infl = (R, CR.distinct_profile(R), FREE)
    for bat in bats:
        bat.set_occupancy([(l, o, res, CR.OUTSIDE, 128) for l, o in zip(layers, origins)], infl, map_of, weight)
    return origins


def cell_pose(twin, m, e, frac=(0.5, 0.5)):
    """a pose whose cell is e = (ex, ey) cells from the centre cell of map m as the twin has it"""
    frame, geo = twin.frame(m)
    return FR.pose_for(frame, geo, (geo[2] // 2 + e[0], geo[3] // 2 + e[1]), frac)


# 1. from scratch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 1, 3))
@pytest.mark.parametrize("nx,ny", ((1, 1), (5, 4), (7, 7), (63, 64), (64, 65), (129, 70)))
def test_two_calls_from_scratch_equal_the_twin(pair7, nx, ny, R):
    """seven robots on maps of their own.  Call one (margin 2, max_step 5): the centre; |e| at the margin; margin + 1; both axes
    with opposite signs; far away, clamped; left of and below the map, on a cell edge; a NaN pose.  Call two, the entries
    reversed (margin 0, max_step 200, fill 255): +-1 on one axis and on both; |d| >= nx and >= ny, every cell exposed; the
    centre; far away once more."""
    bat, tw = pair7
    map_of = list(range(7))
    origins = install((bat, tw), [layer(nx, ny, 10 * R + m) for m in range(7)], R, map_of)
    twin = Twin(tw, origins, RES, map_of)
    bat.resident_set_follow(True)
    assert bat.resident_get_follow() and not tw.resident_get_follow()
    twin.holds(bat)   # (nothing followed yet: status 0)
    e1 = [(0, 0), (2, -2), (3, 0), (-3, 3), (40, 1), (-nx // 2 - 2, -ny // 2 - 1), None]
    xy = [cell_pose(twin, m, e, (0.0, 0.0) if m == 5 else (0.5, 0.5)) if e is not None else (np.nan, 2.0) for m, e in enumerate(e1)]
    set_poses((bat, tw), xy)
    bat.resident_follow(list(range(7)), 2, 5)
    got = twin.follow(list(range(7)), 2, 5)
    assert got == [FR.HELD, FR.HELD, FR.MOVED, FR.MOVED, FR.MOVED, FR.MOVED, FR.NO_POSE]
    assert twin.shift[2:5].tolist() == [[3, 0], [-3, 3], [5, 0]] and twin.shift[5, 0] == max(-5, -nx // 2 - 2)
    twin.holds(bat)
    e2 = [(1, 0), (0, -1), (-1, 1), (nx + 3, 0), (0, -(ny + 2)), (0, 0), (-500, 500)]
    xy = [cell_pose(twin, m, e) for m, e in enumerate(e2)]
    set_poses((bat, tw), xy)   # (finite poses again: the tick reads the grid rows the first call wrote)
    same_tick(bat, tw, 2)
    twin.holds(bat)
    order = list(range(6, -1, -1))
    bat.resident_follow(order, 0, 200, 255)
    got = twin.follow(order, 0, 200, 255)
    assert got == [FR.MOVED, FR.HELD, FR.MOVED, FR.MOVED, FR.MOVED, FR.MOVED, FR.MOVED]
    assert twin.shift[3].tolist() == [nx + 3, 0] and twin.shift[6].tolist() == [-200, 200]
    assert (tw.read_occupancy(3) == 255).all() and (tw.read_occupancy(6) == 255).all()   # (every cell exposed)
    twin.holds(bat)
    same_tick(bat, tw, 3)
    twin.holds(bat)


def test_twelve_calls_at_a_resolution_that_rounds_equal_the_twin(pair3):
    """0.05 m cells and origins that are no multiples of them: (x - origin) * inv and origin0 + c * resolution round on the
    device, so a contracted operation or an origin formed by repeated addition would show.  The robots stand at cell centres 30,
    17 and 5 cells from the centre cells; margin 0, max_step 3: ten, six and ten calls that move, then HELD."""
    bat, tw = pair3
    res, map_of = 0.05, [0, 1, 2]
    origins = install((bat, tw), [layer(9, 7, 70 + m) for m in range(3)], 1, map_of, res=res, origins=[(2.23, 0.81), (-1.37, -4.19), (0.07, 0.03)])
    twin = Twin(tw, origins, res, map_of)
    bat.resident_set_follow(True)
    set_poses((bat, tw), [cell_pose(twin, 0, (30, -17)), cell_pose(twin, 1, (-17, 5)), cell_pose(twin, 2, (5, 30))])
    moves = [0, 0, 0]
    for call in range(12):
        bat.resident_follow([0, 1, 2], 0, 3)
        got = twin.follow([0, 1, 2], 0, 3)
        moves = [a + (g == FR.MOVED) for a, g in zip(moves, got)]
        twin.holds(bat)
        same_tick(bat, tw, 30 + call)
    assert moves == [10, 6, 10] and twin.c.tolist() == [[30, -17], [-17, 5], [5, 30]]
    exact = [(o[0] + float(c[0]) * res, o[1] + float(c[1]) * res) for o, c in zip(origins, twin.c)]
    summed = [o[0] for o in origins]
    for _ in range(10):
        summed[0] += 3.0 * res
    assert [g[0] for g in bat.get_occupancy()] == exact and summed[0] != exact[0][0]   # (the cases tell a running sum from the statement)


# 2. call mixes ------------------------------------------------------------------------------------------------------------------
def test_call_mixes_equal_the_twin(pair3):
    """two calls in a row (the frame slots return to where they started), a HELD call between two MOVED ones, a patch and a scan
    after a follow (the rolled frame is addressed), one entry, a call that names only some of the maps: the others keep every
    bit, and so do their instances' ticks."""
    bat, tw = pair3
    map_of = [0, 1, 2]
    nx, ny, R = 9, 7, 2
    origins = install((bat, tw), [layer(nx, ny, 40 + m) for m in range(3)], R, map_of)
    twin = Twin(tw, origins, RES, map_of)
    bat.resident_set_follow(True)
    set_poses((bat, tw), [cell_pose(twin, 0, (3, 0)), cell_pose(twin, 1, (0, -4)), cell_pose(twin, 2, (6, 6))])
    for call in range(4):   # map 0: MOVED then HELD; map 1: MOVED, MOVED (max_step 2), HELD; map 2: MOVED three times, then HELD
        bat.resident_follow([0, 1, 2], 1, 2)
        got = twin.follow([0, 1, 2], 1, 2)
        assert got == [[FR.MOVED] * 3, [FR.HELD, FR.MOVED, FR.MOVED], [FR.HELD, FR.HELD, FR.MOVED], [FR.HELD] * 3][call], (call, got)
        twin.holds(bat)
        same_tick(bat, tw, 10 + call)
    # a HELD call between two MOVED ones, one entry
    set_poses((bat, tw), [cell_pose(twin, 0, (-2, 0)), cell_pose(twin, 1, (0, 0)), cell_pose(twin, 2, (0, 0))])
    bat.resident_follow([0], 1, 9)
    assert twin.follow([0], 1, 9) == [FR.MOVED]
    same_tick(bat, tw, 20)
    bat.resident_follow([0], 1, 9)
    assert twin.follow([0], 1, 9) == [FR.HELD]
    twin.holds(bat)
    same_tick(bat, tw, 21)
    set_poses((bat, tw), [cell_pose(twin, 0, (0, 3)), cell_pose(twin, 1, (0, 0)), cell_pose(twin, 2, (0, 0))])
    bat.resident_follow([0], 1, 9, 200)
    assert twin.follow([0], 1, 9, 200) == [FR.MOVED]
    twin.holds(bat)
    same_tick(bat, tw, 22)
    # a patch and a scan address the rolled frame
    patch = np.array([[255, 0, 255], [0, 255, 0]], dtype=np.uint8)
    ends = np.array([[8, 6], [0, 0], [12, 3]], dtype=np.int32)
    for h in (bat, tw):
        h.update_occupancy(0, 2, 1, patch)
        h.scan_occupancy([2], [(4, 3)], [ends], [np.array([1, 0, 1])])
    twin.holds(bat)
    # only some of the maps, reversed: map 1 and its robot keep every bit
    before = (bat.read_occupancy(1).tobytes(), derived(bat, 1).tobytes(), bat.get_occupancy()[1])
    set_poses((bat, tw), [cell_pose(twin, 0, (2, 2)), cell_pose(twin, 1, (5, 5)), cell_pose(twin, 2, (-3, 0))])
    bat.resident_follow([2, 0], 0, 3)
    assert twin.follow([2, 0], 0, 3) == [FR.MOVED, FR.MOVED]
    assert before == (bat.read_occupancy(1).tobytes(), derived(bat, 1).tobytes(), bat.get_occupancy()[1])
    twin.holds(bat)
    same_tick(bat, tw, 5)


# 3. set and unset ---------------------------------------------------------------------------------------------------------------
def test_unset_after_moves_gives_the_maps_back_to_the_host(pair3):
    bat, tw = pair3
    map_of = [0, 1, 1]   # (two robots on map 1: only one of them may be named)
    origins = install((bat, tw), [layer(12, 10, 50), layer(6, 8, 51)], 1, map_of)
    twin = Twin(tw, origins, RES, map_of)
    with pytest.raises(Exception):
        BatchController.resident_follow(bat, [0], 1, 2)   # (following is not set)
    bat.resident_set_follow(True)
    set_poses((bat, tw), [cell_pose(twin, 0, (4, -3)), cell_pose(twin, 1, (-2, 2)), cell_pose(twin, 1, (0, 0))])
    bat.resident_follow([0, 1], 1, 3)
    assert twin.follow([0, 1], 1, 3) == [FR.MOVED, FR.MOVED]
    moved = bat.get_occupancy()
    assert moved == tw.get_occupancy() and moved[0][0] == (origins[0][0] + 3.0 * RES, origins[0][1] - 3.0 * RES)
    # a host roll is refused while the maps follow, and nothing changes
    m = np.array([0], dtype=np.int32)
    rc = bat.lib.ccv_mppi_batch_roll_occupancy_enqueue(bat._h, 1, m.ctypes.data_as(i32p), m.ctypes.data_as(i32p), m.ctypes.data_as(i32p), None, 0)
    assert rc == capi.ERR_STATE
    twin.holds(bat)
    bat.resident_set_follow(False)
    assert not bat.resident_get_follow() and bat.get_occupancy() == moved
    assert bat.lib.ccv_mppi_batch_resident_read_follow(bat._h, None, None, None, None) == capi.ERR_STATE
    twin.holds(bat, rows=False)
    same_tick(bat, tw, 2)
    for h in (bat, tw):   # host rolls work again, from the frame the device left
        h.roll_occupancy([0, 1], [-2, 1], [1, 0], None, 77)
    twin.c += [[-2, 1], [1, 0]]
    twin.holds(bat, rows=False)
    # ... and following starts again from the frame the host rolled to
    bat.resident_set_follow(True)
    twin.status[:], twin.shift[:] = 0, 0
    twin.holds(bat)
    bat.resident_follow([2], 0, 1)
    assert twin.follow([2], 0, 1) == [FR.MOVED]
    twin.holds(bat)
    # _set_occupancy drops following
    install((bat, tw), [layer(12, 10, 50), layer(6, 8, 51)], 1, map_of)
    assert not bat.resident_get_follow()


# 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pair3):
    bat, tw = pair3
    lib = bat.lib

    def call(inst, margin=1, max_step=2, fill=0, n=None):
        a = np.array(inst, dtype=np.int32)
        return lib.ccv_mppi_batch_resident_follow_enqueue(bat._h, len(a) if n is None else n, a.ctypes.data_as(i32p), margin, max_step, fill)

    for h in (bat, tw):
        h.set_occupancy(None)
    assert lib.ccv_mppi_batch_resident_set_follow(bat._h, 1) == capi.ERR_STATE   # (no occupancy)
    map_of = [0, 1, -1]
    origins = install((bat, tw), [layer(8, 8, 60), layer(8, 8, 61)], 2, map_of)
    twin = Twin(tw, origins, RES, map_of)
    set_poses((bat, tw), [cell_pose(twin, 0, (3, 0)), cell_pose(twin, 1, (0, 3)), (0.0, 0.0)])
    assert call([0]) == capi.ERR_STATE   # (following is not set)
    inst, goal = np.array([0], dtype=np.int32), np.array([[0.0, 0.0]])
    for h in (bat, tw):
        h.resident_set_plan(16)
    assert lib.ccv_mppi_batch_resident_plan_goals_enqueue(bat._h, 1, inst.ctypes.data_as(i32p), capi.dptr(goal), 0.5, 10) == capi.ERR_STATE
    assert b"resident_plan_goals: following is not set" in lib.ccv_mppi_batch_last_error(bat._h)
    assert bat.resident_read_plan()[0].tolist() == [0, 0, 0]
    twin.holds(bat, rows=False)   # (neither refusal changed a bit of a map that is not followed)
    same_tick(bat, tw, 7)
    bat.resident_set_follow(True)
    G = 32768   # CCV_MPPI_GRID_MAX_DIM
    for rc in (call([0], n=0), call([0, 1, 0, 1], n=4), call([3]), call([-1]), call([0, 0]), call([2]), call([0], margin=-1), call([0], margin=G + 1),
               call([0], max_step=0), call([0], max_step=G + 1), call([0], fill=-1), call([0], fill=256),
               lib.ccv_mppi_batch_resident_follow_enqueue(bat._h, 1, None, 1, 2, 0)):
        assert rc == capi.ERR_INVALID_ARG, lib.ccv_mppi_batch_last_error(bat._h)
    # the poses would move both maps, and no refusal changed a bit: layers, cells, origins, status 0 in every row, the next tick
    twin.holds(bat)
    same_tick(bat, tw, 8)
    twin.holds(bat)
    bat.resident_follow([0, 1], 1, 2)   # (... and the first call that is taken does move them)
    assert twin.follow([0, 1], 1, 2) == [FR.MOVED, FR.MOVED]
    twin.holds(bat)
    same_tick(bat, tw, 9)
    # two named instances on one map
    for h in (bat, tw):
        h.set_occupancy([(layer(8, 8, 60), origins[0], RES, CR.OUTSIDE, 128), (layer(8, 8, 61), origins[1], RES, CR.OUTSIDE, 128)],
                        (2, CR.distinct_profile(2), FREE), [0, 1, 1], 1.0)
    twin = Twin(tw, origins, RES, [0, 1, 1])
    bat.resident_set_follow(True)
    assert call([1, 2]) == capi.ERR_INVALID_ARG
    goals = np.array([[np.inf, 0.0]])
    twin.holds(bat)   # (no refusal changed a bit, and no map counts as followed)
    same_tick(bat, tw, 1)
    # no resident poses: a handle that has paths only
    fresh = make(2)
    try:
        fresh.set_occupancy([(layer(4, 4, 1), ORIGIN, RES, CR.OUTSIDE, 128)], (1, CR.distinct_profile(1), FREE), [0, 0], 1.0)
        fresh.resident_set_follow(True)
        a = np.array([0], dtype=np.int32)
        assert lib.ccv_mppi_batch_resident_follow_enqueue(fresh._h, 1, a.ctypes.data_as(i32p), 1, 2, 0) == capi.ERR_STATE
        fresh.resident_set_poses(np.zeros((2, 3)), 1)
        fresh.resident_set_plan(16)
        assert lib.ccv_mppi_batch_resident_plan_goals_enqueue(fresh._h, 1, a.ctypes.data_as(i32p), capi.dptr(goals), 0.5, 10) == capi.ERR_INVALID_ARG
        assert lib.ccv_mppi_batch_resident_plan_goals_enqueue(fresh._h, 1, a.ctypes.data_as(i32p), None, 0.5, 10) == capi.ERR_INVALID_ARG
    finally:
        fresh.close()


def test_a_table_above_one_staging_slot_is_refused():
    """a slot has CCV_MPPI_OCC_PATCH_MAX_CELLS bytes and an entry 192: the first count that does not fit is 5 462"""
    n = capi.OCC_PATCH_MAX_CELLS // 192 + 1
    bat = make(n)
    try:
        cells = layer(6, 6, 3)
        bat.set_occupancy([(cells, ORIGIN, RES, CR.OUTSIDE, 128)], (1, CR.distinct_profile(1), FREE), np.zeros(n, dtype=np.int32), 1.0)
        bat.resident_set_poses(np.zeros((n, 3)), 1)
        bat.resident_set_follow(True)
        inst = np.arange(n, dtype=np.int32)
        assert bat.lib.ccv_mppi_batch_resident_follow_enqueue(bat._h, n, inst.ctypes.data_as(i32p), 1, 2, 0) == capi.ERR_INVALID_ARG
        assert b"staging slot" in bat.lib.ccv_mppi_batch_last_error(bat._h)
        assert bat.resident_read_follow()[0].tolist() == [0] and same(bat.read_occupancy(0), cells)
        bat.resident_follow([n - 1], 0, 1)   # (one entry of the same handle is fine)
        assert bat.resident_read_follow()[0].tolist() == [FR.MOVED]
    finally:
        bat.close()


# 5. memory ----------------------------------------------------------------------------------------------------------------------
def test_forty_set_and_unset_cycles_return_all_device_memory(pair3):
    import torch
    bat, tw = pair3
    map_of = [0, 1, 2]
    origins = install((bat,), [layer(64, 64, m) for m in range(3)], 2, map_of)
    set_poses((bat,), [(origins[m][0] + 5.0, origins[m][1] + 5.0) for m in range(3)])

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        bat.resident_set_follow(True)
        bat.resident_follow([0, 1, 2], 1, 4)
        bat.resident_set_follow(False)

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)


# 6. the closed loop -------------------------------------------------------------------------------------------------------------
def test_forty_ticks_of_a_following_fleet_equal_a_twin_that_decides_on_the_host():
    """Three robots drive straight paths through a walled world, each with a 20 x 20 map (R = 2) round it: every tick the maps
    follow (margin 2), every second tick the robots sense, every fifth they plan to a fixed world goal.  The twin reads its poses
    back every tick, decides with the checker and rolls; it turns the goal into a cell with batch.goal_cells against the origin
    it reads.  It runs first and counts on its own read-backs what the run has to show."""
    res, nx, ny, R, ticks, cap = 0.0625, 20, 20, 2, 40, 64
    wo = (-2.0, -2.0)
    world = np.zeros((160, 160), dtype=np.uint8)
    world[0, :] = world[-1, :] = world[:, 0] = world[:, -1] = 255
    world[40:120, 100] = 255          # (a wall across robot 0's way, far enough not to be reached)
    world[70:74, 20:60] = 255         # (... and a block beside robot 1's)
    starts = [(30, 30), (64, 40), (40, 90)]                       # world cells
    headings = [0.0, 0.5 * np.pi, 0.25 * np.pi]
    s0 = np.zeros((3, 3))
    for b, (c, h) in enumerate(zip(starts, headings)):
        s0[b] = (wo[0] + (c[0] + 0.5) * res, wo[1] + (c[1] + 0.5) * res, h)
    seeds = np.array([BS.instance_seed(b) for b in range(3)], dtype=np.uint64)
    paths = [(s0[b, 0] + res * np.cos(headings[b]) * np.arange(300.0), s0[b, 1] + res * np.sin(headings[b]) * np.arange(300.0)) for b in range(3)]
    anchors = [(c[0] - nx // 2, c[1] - ny // 2) for c in starts]
    origins = [(wo[0] + a[0] * res, wo[1] + a[1] * res) for a in anchors]
    infl = batch.inflation_profile(2 * res, res)
    assert infl[0] == R
    beams = batch.beam_fan(48, 8)
    goal = np.array([[wo[0] + 3.0, wo[1] + 2.0], [wo[0] + 4.2, wo[1] + 4.4], [wo[0] + 3.1, wo[1] + 6.2]])   # far: clamped at first
    lethal = 0.5

    def make_loop():
        bat = BatchController(P, 3)
        bat.resident_set_paths(paths, res)
        bat.resident_set_poses(s0, seeds)
        bat.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), o, res, 0.0, 128) for o in origins], infl, [0, 1, 2], 2.0)
        bat.set_world(world, 128, wo, res, anchors, len(beams))
        bat.resident_set_plan(cap, False)
        return bat

    def leaves(bat):
        out = [bat.resident_read_trace(b).tobytes() for b in range(3)] + CS.tick_bits(bat)
        out += [bat.read_occupancy(m).tobytes() + derived(bat, m).tobytes() for m in range(3)]
        out += [a.tobytes() for a in bat.resident_read_sense()] + [a.tobytes() for a in bat.resident_read_plan()]
        out += [np.concatenate(bat.resident_read_path(b)).tobytes() for b in range(3)]
        return out + [repr(bat.get_occupancy())]

    tw = make_loop()
    twin = Twin(tw, origins, res, [0, 1, 2])
    tw.roll_occupancy([0, 1, 2], 0, 0)
    counts = np.zeros((3, 5), dtype=np.int64)
    clamped = ok = 0
    for t in range(ticks):
        tw.resident_step_enqueue(P.dt, t)
        for b, s in enumerate(twin.follow([0, 1, 2], 2, 3)):
            counts[b, s] += 1
        if t % 2 == 1:
            tw.resident_sense([0, 1, 2], beams)
        if t % 5 == 4:
            geo = tw.get_occupancy()
            cells = np.concatenate([batch.goal_cells((geo[m][0], res, nx, ny), goal[m:m + 1]) for m in range(3)])
            for m in range(3):
                f = (goal[m] - np.array(geo[m][0])) * (1.0 / res)
                clamped += bool((f < 0).any() or (f >= (nx, ny)).any())
            tw.resident_plan([0, 1, 2], cells, lethal)
            ok += int(np.count_nonzero(tw.resident_read_plan()[0] == capi.PLAN_OK))
    print("follow statuses per robot (columns 0..4):", counts.tolist(), "offsets:", twin.c.tolist(), "clamped goals:", clamped, "plans OK:", ok)
    assert (counts[:, FR.MOVED] >= 1).all() and (counts[:, FR.HELD] >= 1).all(), counts
    assert (np.abs(twin.c) >= nx).any(), twin.c
    assert clamped >= 1 and ok >= 1, (clamped, ok)
    want = leaves(tw)
    # the following fleet: nothing is read until the last tick has been enqueued
    bat = make_loop()
    try:
        bat.resident_set_follow(True)
        for t in range(ticks):
            bat.resident_step_enqueue(P.dt, t)
            bat.resident_follow([0, 1, 2], 2, 3)
            if t % 2 == 1:
                bat.resident_sense([0, 1, 2], beams)
            if t % 5 == 4:
                bat.resident_plan_goals([0, 1, 2], goal, lethal, nx * ny + 1)
        got = leaves(bat)
        assert len(got) == len(want)
        assert [i for i, (x, y) in enumerate(zip(got, want)) if x != y] == []
        status, shift, offset, origin = bat.resident_read_follow()
        assert status.tolist() == twin.status.tolist() and shift.tolist() == twin.shift.tolist() and offset.tolist() == twin.c.tolist()
    finally:
        BS.close_all(bat, tw)

"""GPU tests (-m gpu) of the weighted device planner (ccv_mppi_batch_resident_set_plan_penalty; BatchController.
resident_set_plan_penalty).

The contract is in integers but for the planner's two floating-point steps and one fp32 multiplication per cell, and the field is
the one fixpoint of its relaxation whatever the device's order, so everything -- field, status, L, D(start), start cell and every
bit of the path -- is held against tests/plan_cost_reference.py with no tolerance.  `sweeps` is the device's own, held inside
[1, J]; where all strips of a map fit one wave (nx + ny <= 64) the lanes run in lockstep and two runs of one kernel take the
same sweeps, which the device-to-device comparison uses.  The unweighted plan the device is compared with is the same handle's
own.  No test asserts a time or looks into a kernel's assembly."""
import ctypes as C

import numpy as np
import pytest

import batch_support as BS
import costmap_support as CS
import follow_reference as FR
import plan_cost_reference as PC
import plan_reference as PR
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import same

pytestmark = pytest.mark.gpu
i32p = C.POINTER(C.c_int32)
ORIGIN, RES, LETHAL = PR.ORIGIN, PR.RES, PR.LETHAL
B = 7
CAP = 1024
GAIN = float(np.float32(8.0 / float(LETHAL)))
KINDS = ("empty", "random", "wall_with_gap", "serpentine")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.fixture(scope="module")
def fleet():
    bat = BatchController(configs.diff_drive_defaults(128, 15), B)
    yield bat
    bat.close()


def pose_at(cell, frac=(0.5, 0.5), origin=ORIGIN):
    return (origin[0] + (cell[0] + frac[0]) * RES, origin[1] + (cell[1] + frac[1]) * RES)


def line_paths(n=(5, 9, 3, 7, 4, 6, 8)):
    return [(ORIGIN[0] + RES * np.arange(k, dtype=np.float64), np.full(k, ORIGIN[1] + 0.1 * b)) for b, k in enumerate(n)]


def install(bat, maps, map_of, poses, capacity=CAP, keep=True, occupancy=None):
    """float maps through _set_grids, or (occupancy = (layers, inflation)) device-inflated ones; planning set: the penalty is
    (0, 0) again.  Returns the paths the instances start with and the float cells per map as the device holds them."""
    paths = line_paths()
    bat.resident_set_paths(paths, RES)
    st = np.zeros((bat.B, 3))
    st[:len(poses), :2] = np.asarray(poses, dtype=np.float64)
    bat.resident_set_poses(st, np.arange(1, bat.B + 1, dtype=np.uint64))
    if occupancy is None:
        bat.set_grids([(m, ORIGIN, RES, 0.0) for m in maps], np.asarray(map_of, dtype=np.int32), 1.0)
    else:
        layers, infl = occupancy
        bat.set_occupancy([(l, ORIGIN, RES, 0.0, 128) for l in layers], infl, np.asarray(map_of, dtype=np.int32), 1.0)
        maps = [g[0] for g in bat.get_grids()[0]]
    bat.resident_set_plan(capacity, keep)
    assert bat.resident_get_plan_penalty() == (0.0, 0)
    return [(np.array(x), np.array(y)) for x, y in paths], maps


def expect(maps, map_of, poses, goals, instances, capacity, gain, maxp, converged=True, origin=ORIGIN):
    cap = np.broadcast_to(np.asarray(capacity), (B,))
    fields = {}   # one field per (map, goal): instances that share both share the checker's work

    def field(m, g):
        if (m, tuple(g)) not in fields:
            fields[(m, tuple(g))] = PC.field_dijkstra(maps[m], g, LETHAL, gain, maxp)
        return fields[(m, tuple(g))]

    return {b: PC.plan(maps[map_of[b]], origin, RES, poses[b], g, LETHAL, int(cap[b]), gain, maxp, converged=converged,
                       field=field(map_of[b], g) if converged else None) for b, g in zip(instances, goals)}


def holds(bat, want, paths, maps, map_of, jacobi=None):
    """every named instance's read-back is the checker's; every path, planned or not, is what it has to be (paths is updated)"""
    status, poses, cell, dist, sweeps = bat.resident_read_plan()
    for b, r in want.items():
        got = (int(status[b]), int(poses[b]), tuple(cell[b].tolist()), int(dist[b]))
        assert got == (r["status"], r["poses"], tuple(r["start"]), r["dist"]), (b, got, r["status"], r["poses"], r["start"], r["dist"])
        if r["path"] is not None:
            paths[b] = r["path"]
        ny, nx = maps[map_of[b]].shape
        if r["field"] is not None:
            got_field = bat.resident_read_plan_field(b, (ny, nx))
            assert same(got_field, r["field"]), (b, np.argwhere(got_field != r["field"])[:4].tolist())
            assert 1 <= sweeps[b] <= nx * ny + 1 and (jacobi is None or sweeps[b] <= jacobi[b]), (b, sweeps[b])
        elif r["status"] != PR.NOT_CONVERGED:
            assert sweeps[b] == 0
    for b in range(bat.B):
        x, y = bat.resident_read_path(b)
        assert same(x, paths[b][0]) and same(y, paths[b][1]), (b, len(x), len(paths[b][0]))


def snapshot(bat, shapes, with_sweeps=True):
    """every read-back of the plan as bytes"""
    rows = bat.resident_read_plan()
    out = [a.tobytes() for a in (rows if with_sweeps else rows[:4])]
    out += [a.tobytes() for b in range(bat.B) for a in bat.resident_read_path(b)]
    return out + [bat.resident_read_plan_field(b, shapes[b]).tobytes() for b in range(bat.B) if rows[0][b] in (1, 2, 6)]


def graded_cases(nx, ny, seed):
    cases = [PR.case(k, nx, ny, seed=seed, finite=True) for k in KINDS]
    return [(PC.graded(c, seed=seed + i), s, g) for i, (c, s, g) in enumerate(cases)]


# 1. from scratch ---------------------------------------------------------------------------------------------------------------------
# the follower's sizes: a pitch nx + 1 of every residue mod 4, one and more than one strip per thread's turn, a single cell
SHAPES = ((1, 1), (5, 4), (7, 7), (63, 64), (64, 65), (129, 70))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_a_weighted_plan_equals_the_checker_from_scratch(fleet, nx, ny):
    """seven instances on four kinds of graded map, three maps shared by two instances: float maps of _set_grids first, then the
    same obstacles as occupancy layers that the device inflates with a graded profile"""
    cases = graded_cases(nx, ny, nx + 3 * ny)
    map_of = [0, 1, 2, 3, 0, 1, 2]
    named = list(range(B))
    for source in ("grids", "occupancy"):
        maps = [c[0] for c in cases]
        occupancy = None
        if source == "occupancy":
            occupancy = ([np.where(PR.blocked(m, LETHAL), 255, 0).astype(np.uint8) for m in maps], batch.inflation_profile(0.75, RES))
        starts = [cases[m][1] if b < 4 else PR.free_cell(maps[m], LETHAL, (3 * nx // 4, ny // 3)) for b, m in enumerate(map_of)]
        poses = [pose_at(s, (0.25, 0.75)) for s in starts]
        goals = [cases[m][2] for m in map_of]
        paths, maps = install(fleet, maps, map_of, poses, occupancy=occupancy)
        if source == "occupancy":   # (the linear profile is below lethal from the first ring on: the same cells are blocked)
            assert all((PR.blocked(m, LETHAL) == PR.blocked(c[0], LETHAL)).all() for m, c in zip(maps, cases))
            assert nx * ny < 20 or any(len(np.unique(m)) > 3 for m in maps)
        fleet.resident_set_plan_penalty(GAIN, 15)
        assert fleet.resident_get_plan_penalty() == (GAIN, 15)
        fleet.resident_plan(named, goals, LETHAL)
        want = expect(maps, map_of, poses, goals, named, CAP, GAIN, 15)
        holds(fleet, want, paths, maps, map_of)
        if nx * ny > 40:
            assert any(want[b]["status"] in (PR.OK, PR.TRUNCATED) for b in named)
            assert any((want[b]["field"] != PR.field_dijkstra(maps[b], goals[b], LETHAL)).any() for b in (1, 2)), source   # (the weights matter here)


def test_the_widest_image_whose_pitch_cannot_be_padded(fleet):
    nx, ny = 318, 254   # (nx + 2)(ny + 2) = CCV_MPPI_PLAN_MAX_FIELD
    cells = PC.graded(PR.case("wall_with_gap", nx, ny, finite=True)[0], seed=1)
    start, goal = (0, 0), (nx - 1, ny - 1)
    map_of = [0] * B
    poses = [pose_at(start), pose_at((nx - 1, 0), (0.9, 0.1))] + [pose_at(start)] * (B - 2)
    paths, maps = install(fleet, [cells], map_of, poses)
    fleet.resident_set_plan_penalty(GAIN, 15)
    fleet.resident_plan([0, 1], [goal, goal], LETHAL)
    D = PC.field_dijkstra(cells, goal, LETHAL, GAIN, 15)   # (one field for both: the checker's time)
    want = {b: PC.plan(cells, ORIGIN, RES, poses[b], goal, LETHAL, CAP, GAIN, 15, field=D) for b in (0, 1)}
    assert want[0]["status"] in (PR.OK, PR.TRUNCATED) and want[0]["dist"] > 5 * nx
    holds(fleet, want, paths, maps, map_of)


# 2. zero penalties: the unweighted plan of the same handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,lockstep", ((31, 19, True), (64, 65, False)))
def test_zero_penalty_and_zero_gain_are_the_handles_own_unweighted_plan(fleet, nx, ny, lockstep):
    cases = graded_cases(nx, ny, 7)
    maps, map_of = [c[0] for c in cases], [0, 1, 2, 3, 0, 1, 2]
    poses = [pose_at(cases[m][1], (0.1 * b, 0.9 - 0.1 * b)) for b, m in enumerate(map_of)]
    goals = [cases[m][2] for m in map_of]
    shapes = [(ny, nx)] * B
    paths, maps = install(fleet, maps, map_of, poses)
    named = list(range(B))
    fleet.resident_plan(named, goals, LETHAL)
    plain = snapshot(fleet, shapes, lockstep)
    J = [PR.field_jacobi(maps[m], goals[b], LETHAL)[1] for b, m in enumerate(map_of)]
    for gain, maxp in ((GAIN, 0), (0.0, 15), (0.0, 0)):
        fleet.resident_set_plan_penalty(GAIN, 15)
        fleet.resident_plan(named, goals, LETHAL)          # a weighted plan in between: every read-back changes ...
        assert snapshot(fleet, shapes, lockstep) != plain
        fleet.resident_set_plan_penalty(gain, maxp)
        assert fleet.resident_get_plan_penalty() == (gain, maxp)
        fleet.resident_plan(named, goals, LETHAL)          # ... and comes back, device to device
        assert snapshot(fleet, shapes, lockstep) == plain, (gain, maxp)
        sweeps = fleet.resident_read_plan()[4]
        assert all(1 <= sweeps[b] <= J[b] for b in named)


# 3. the spec's cases -----------------------------------------------------------------------------------------------------------------
def test_the_clearance_case(fleet):
    cells, start, goal = PC.clearance_case()
    map_of, poses = [0] * B, [pose_at(start)] * B
    paths, maps = install(fleet, [cells], map_of, poses)
    fleet.resident_plan([0], [goal], LETHAL)
    fleet.resident_set_plan_penalty(8.0, 15)
    fleet.resident_plan([1], [goal], LETHAL)
    want = {0: PC.plan(cells, ORIGIN, RES, poses[0], goal, LETHAL, CAP, 0.0, 0), 1: PC.plan(cells, ORIGIN, RES, poses[1], goal, LETHAL, CAP, 8.0, 15)}
    holds(fleet, want, paths, maps, map_of)
    routes = [PC.route_cells(fleet.resident_read_path(b), ORIGIN, RES) for b in (0, 1)]
    assert routes[0] == [(0, 3), (1, 3), (2, 3), (3, 4), (4, 4), (5, 4), (6, 4), (7, 4), (8, 3)]
    assert routes[1] == [(0, 3), (1, 3), (2, 4), (3, 5), (4, 5), (5, 5), (6, 5), (7, 4), (8, 3)]
    assert fleet.resident_read_plan()[3][:2].tolist() == [44, 48]
    assert sum(cells[y, x] == 0.5 for x, y in routes[0]) == 3 and sum(cells[y, x] == 0.5 for x, y in routes[1]) == 0


def test_the_saturating_row(fleet):
    cells = np.full((1, 900), 0.5, dtype=np.float32)
    map_of = [0] * B
    poses = [pose_at((820, 0)), pose_at((819, 0))] + [pose_at((1, 0))] * (B - 2)
    paths, maps = install(fleet, [cells], map_of, poses)
    fleet.resident_set_plan_penalty(30.0, 15)
    fleet.resident_plan([0, 1, 2], [(0, 0)] * 3, LETHAL)
    want = expect(maps, map_of, poses, [(0, 0)] * 3, [0, 1, 2], CAP, 30.0, 15)
    assert [want[b]["status"] for b in (0, 1, 2)] == [PR.UNREACHABLE, PR.OK, PR.OK]
    assert [want[b]["dist"] for b in (0, 1, 2)] == [PR.FAR, 65520, 80] and want[1]["poses"] == 820
    holds(fleet, want, paths, maps, map_of)
    field = fleet.resident_read_plan_field(0, (1, 900))
    assert field[0, 819] == 65520 and (field[0, 820:] == PR.FAR).all()


def test_a_product_on_an_integer_and_one_float_below_change_the_route(fleet):
    """the corridor's five middle cells at 0.125 (t = 1, m = 2: 5 + 25 * 2 = 55 through them, 34 round them) and one float below
    (t < 1, m = 1: 30 through them)"""
    on = np.zeros((3, 7), dtype=np.float32)
    on[1, 1:6] = 0.125
    under = on.copy()
    under[1, 1:6] = np.nextafter(np.float32(0.125), np.float32(0))
    map_of, poses = [0, 1] + [0] * (B - 2), [pose_at((0, 1))] * B
    paths, maps = install(fleet, [on, under], map_of, poses)
    fleet.resident_set_plan_penalty(8.0, 15)
    fleet.resident_plan([0, 1], [(6, 1)] * 2, LETHAL)
    want = expect(maps, map_of, poses, [(6, 1)] * 2, [0, 1], CAP, 8.0, 15)
    assert [want[b]["dist"] for b in (0, 1)] == [34, 30]
    holds(fleet, want, paths, maps, map_of)
    routes = [PC.route_cells(fleet.resident_read_path(b), ORIGIN, RES) for b in (0, 1)]
    assert all(y != 1 for x, y in routes[0][1:-1]) and all(y == 1 for x, y in routes[1])


# 4. capacities and sweeps ------------------------------------------------------------------------------------------------------------
def test_capacity_l_l_minus_one_and_one(fleet):
    cells = PC.graded(PR.case("wall_with_gap", 63, 64, finite=True)[0], seed=2)
    start, goal = (0, 0), (62, 63)
    L = PC.plan(cells, ORIGIN, RES, pose_at(start), goal, LETHAL, PR.MAX_POSES, GAIN, 15)["poses"]
    assert L > 60
    cap = np.array([L, L - 1, 1, L + 1, 0, PR.MAX_POSES, 2], dtype=np.int32)
    map_of, poses = [0] * B, [pose_at(start)] * B
    paths, maps = install(fleet, [cells], map_of, poses, capacity=cap)
    fleet.resident_set_plan_penalty(GAIN, 15)
    named = [0, 1, 2, 3, 5, 6]
    fleet.resident_plan(named, [goal] * 6, LETHAL)
    want = expect(maps, map_of, poses, [goal] * 6, named, cap, GAIN, 15)
    assert [want[b]["status"] for b in named] == [PR.OK, PR.TRUNCATED, PR.TRUNCATED, PR.OK, PR.OK, PR.TRUNCATED]
    assert [len(want[b]["path"][0]) for b in named] == [L, L - 1, 1, L, L, 2] and all(want[b]["poses"] == L for b in named)
    holds(fleet, want, paths, maps, map_of)


def test_max_sweeps_the_weighted_j_converges_and_one_does_not(fleet):
    cases = graded_cases(23, 17, 2)
    maps, map_of = [c[0] for c in cases], [0, 1, 2, 3, 0, 1, 2]
    poses = [pose_at(cases[m][1]) for m in map_of]
    goals = [cases[m][2] for m in map_of]
    J = [PC.field_jacobi(maps[m], goals[b], LETHAL, GAIN, 15)[1] for b, m in enumerate(map_of)]
    assert max(J) > 40 and min(J) > 2
    paths, maps = install(fleet, maps, map_of, poses)
    fleet.resident_set_plan_penalty(GAIN, 15)
    inst = lambda a: np.array(a, dtype=np.int32).ctypes.data_as(i32p)
    for b in range(4):   # one call per J: max_sweeps is the call's
        assert fleet.lib.ccv_mppi_batch_resident_plan_enqueue(fleet._h, 1, inst([b]), inst(goals[b]), float(LETHAL), J[b]) == capi.OK
    want = expect(maps, map_of, poses, goals[:4], range(4), CAP, GAIN, 15)
    assert all(want[b]["status"] in (PR.OK, PR.UNREACHABLE) for b in range(4))
    holds(fleet, want, paths, maps, map_of, jacobi=J)
    assert fleet.lib.ccv_mppi_batch_resident_plan_enqueue(fleet._h, 3, inst([4, 5, 6]), inst(goals[4:]), float(LETHAL), 1) == capi.OK
    want = expect(maps, map_of, poses, goals[4:], [4, 5, 6], CAP, GAIN, 15, converged=False)
    holds(fleet, want, paths, maps, map_of)
    status, _, _, _, sweeps = fleet.resident_read_plan()
    assert (status[[4, 5, 6]] == PR.NOT_CONVERGED).all() and (sweeps[[4, 5, 6]] == 1).all()


# 5. refusals, and what drops the setting ---------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_the_setting_goes_with_planning():
    p = configs.diff_drive_defaults(128, 15)
    bat = BatchController(p, B)
    lib = bat.lib
    g, m = C.c_float(-1.0), C.c_int32(-1)
    try:
        cells, start, goal = PC.clearance_case()
        bat.resident_set_paths(line_paths(), RES)
        assert lib.ccv_mppi_batch_resident_set_plan_penalty(bat._h, 8.0, 15) == capi.ERR_STATE      # before _set_plan
        assert lib.ccv_mppi_batch_resident_get_plan_penalty(bat._h, C.byref(g), C.byref(m)) == capi.ERR_STATE
        assert (g.value, m.value) == (-1.0, -1)
        paths, maps = install(bat, [cells], [0] * B, [pose_at(start)] * B)
        bat.resident_set_plan_penalty(8.0, 15)
        bat.resident_plan([0, 1], [goal] * 2, LETHAL)
        shapes = [cells.shape] * B
        before = snapshot(bat, shapes)
        for gain, maxp in ((np.nan, 15), (np.inf, 15), (-np.inf, 15), (-1.0, 15), (-1e-30, 3), (8.0, -1), (8.0, 16), (np.nan, 99)):
            assert lib.ccv_mppi_batch_resident_set_plan_penalty(bat._h, gain, maxp) == capi.ERR_INVALID_ARG, (gain, maxp)
            assert b"resident_set_plan_penalty" in lib.ccv_mppi_batch_last_error(bat._h)
            assert bat.resident_get_plan_penalty() == (8.0, 15)
        assert snapshot(bat, shapes) == before
        bat.resident_plan([0, 1], [goal] * 2, LETHAL)      # (... and the next plan is the weighted one still)
        assert snapshot(bat, shapes) == before and bat.resident_read_plan()[3][:2].tolist() == [48, 48]
        assert lib.ccv_mppi_batch_resident_get_plan_penalty(bat._h, None, None) == capi.OK
        assert lib.ccv_mppi_batch_resident_get_plan_penalty(bat._h, None, C.byref(m)) == capi.OK and m.value == 15
        # the edges that are taken: -0.0, the largest float, the smallest subnormal, max_penalty 0 and 15
        tiny = float(np.nextafter(np.float32(0), np.float32(1)))
        for gain, maxp in ((-0.0, 15), (float(np.finfo(np.float32).max), 15), (tiny, 15), (8.0, 0), (0.0, 0)):
            bat.resident_set_plan_penalty(gain, maxp)
            assert bat.resident_get_plan_penalty() == (gain, maxp)
            bat.resident_plan([0], [goal], LETHAL)
            want = PC.plan(cells, ORIGIN, RES, pose_at(start), goal, LETHAL, CAP, gain, maxp)
            assert bat.resident_read_plan()[3][0] == want["dist"] and same(bat.resident_read_plan_field(0, cells.shape), want["field"]), (gain, maxp)
        # a second _set_plan, _set_plan(NULL) and _resident_set_paths drop the setting
        bat.resident_set_plan_penalty(8.0, 15)
        bat.resident_set_plan(64, True)
        assert bat.resident_get_plan_penalty() == (0.0, 0)
        bat.resident_set_plan_penalty(3.0, 7)
        bat.resident_set_plan(None)
        assert lib.ccv_mppi_batch_resident_set_plan_penalty(bat._h, 8.0, 15) == capi.ERR_STATE
        assert lib.ccv_mppi_batch_resident_get_plan_penalty(bat._h, C.byref(g), C.byref(m)) == capi.ERR_STATE
        bat.resident_set_plan(CAP, True)
        assert bat.resident_get_plan_penalty() == (0.0, 0)
        bat.resident_set_plan_penalty(3.0, 7)
        bat.resident_set_paths(line_paths(), RES)
        assert lib.ccv_mppi_batch_resident_get_plan_penalty(bat._h, C.byref(g), C.byref(m)) == capi.ERR_STATE
        bat.resident_set_plan(CAP, True)
        assert bat.resident_get_plan_penalty() == (0.0, 0)
        bat.resident_plan([0], [goal], LETHAL)             # (unweighted again)
        assert bat.resident_read_plan()[3][0] == 44
    finally:
        bat.close()


def test_forty_set_and_unset_cycles_return_all_device_memory(fleet):
    import torch
    cells = PC.graded(PR.wall_with_gap(129, 70), seed=3)
    install(fleet, [cells], [0] * B, [pose_at((1, 1))] * B)

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        fleet.resident_set_plan(CAP, True)
        fleet.resident_set_plan_penalty(GAIN, 15)
        fleet.resident_plan([0, 3], [(120, 60), (3, 60)], LETHAL)
        fleet.resident_set_plan_penalty(0.0, 0)
        fleet.resident_set_plan(None)

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    # (one leaked path array of this layout a cycle would be 4.5 MiB)
    assert abs(free0 - free1) < 4 * 2**20, "device memory changed by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)


# 6. maps that follow, world goals ------------------------------------------------------------------------------------------------------
class Twin:
    """a handle whose maps the host rolls: it reads its poses back, decides with the checker (tests/follow_reference.py) and rolls"""

    def __init__(self, bat, origins0, nx, ny):
        self.bat, self.o0, self.nx, self.ny = bat, [tuple(o) for o in origins0], nx, ny
        self.c = np.zeros((len(origins0), 2), dtype=np.int64)

    def follow(self, instances, margin, max_step):
        st = self.bat.resident_read()[0]
        geo = self.bat.get_occupancy()
        maps, dxs, dys = [], [], []
        for b in instances:   # (instance b is on map b)
            frame = (int(self.c[b, 0]), int(self.c[b, 1]), geo[b][0][0], geo[b][0][1])
            status, dx, dy, new = FR.decide(frame, st[b, :2], (self.o0[b], RES, self.nx, self.ny), margin, max_step)
            if status == FR.MOVED:
                maps.append(b), dxs.append(dx), dys.append(dy)
                self.c[b] = new[:2]
        if maps:
            self.bat.roll_occupancy(maps, dxs, dys, None, 0)


def walled_world():
    """(world, its origin): 120 x 90 cells with a border and a wall at x = 52 with a gap of four cells"""
    world = np.zeros((90, 120), dtype=np.uint8)
    world[0, :] = world[-1, :] = world[:, 0] = world[:, -1] = 255
    world[14:76, 52] = 255
    world[36:40, 52] = 0
    return world, (-2.0, -1.0)


def test_world_goals_after_the_maps_have_moved_equal_the_checker_on_a_twins_read_backs():
    p = configs.diff_drive_defaults(128, 15)
    nx, ny = 48, 40
    world, wo = walled_world()
    starts = [(40, 40), (42, 50), (60, 30)]
    anchors = [(c[0] - nx // 2, c[1] - ny // 2) for c in starts]
    origins = [(wo[0] + a[0] * RES, wo[1] + a[1] * RES) for a in anchors]
    infl = batch.inflation_profile(0.75, RES)
    beams = batch.beam_fan(120, 24)
    s0 = np.zeros((3, 3))
    s0[:, :2] = [pose_at(c, origin=wo) for c in starts]
    moved = s0.copy()
    moved[:, :2] = [pose_at((c[0] + dx, c[1] + dy), (0.3, 0.6), origin=wo) for c, (dx, dy) in zip(starts, ((5, -4), (-6, 3), (0, 7)))]
    goals = np.array([[wo[0] + 70.5 * RES, wo[1] + 37.5 * RES], [wo[0] + 60.2 * RES, wo[1] + 20.4 * RES], [wo[0] - 5.0, wo[1] + 38.0 * RES]])
    lines = [(s0[b, 0] + RES * np.arange(30.0), np.full(30, s0[b, 1])) for b in range(3)]

    def make():
        bat = BatchController(p, 3)
        bat.resident_set_paths(lines, RES)
        bat.resident_set_poses(s0, np.arange(1, 4, dtype=np.uint64))
        bat.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), o, RES, 0.0, 128) for o in origins], infl, [0, 1, 2], 1.0)
        bat.set_world(world, 128, wo, RES, anchors, len(beams))
        bat.resident_set_plan(CAP, True)
        return bat

    bat, tw = make(), make()
    try:
        twin = Twin(tw, origins, nx, ny)
        tw.roll_occupancy([0, 1, 2], 0, 0)
        bat.resident_set_follow(True)
        bat.resident_set_plan_penalty(GAIN, 15)
        for h in (bat, tw):
            h.resident_sense([0, 1, 2], beams)
            h.resident_set_poses(moved, np.arange(1, 4, dtype=np.uint64))
        for _ in range(2):   # (max_step 3: two calls move each map by up to six cells)
            bat.resident_follow([0, 1, 2], 1, 3)
            twin.follow([0, 1, 2], 1, 3)
        for h in (bat, tw):
            h.resident_sense([0, 1, 2], beams)
        bat.resident_plan_goals([0, 1, 2], goals, LETHAL)
        assert (twin.c != 0).any(axis=1).all(), twin.c
        grids = tw.get_grids()[0]
        assert [g[1] for g in grids] == [g[1] for g in bat.get_grids()[0]]
        status, poses, cell, dist, sweeps = bat.resident_read_plan()
        seen, differs = set(), 0
        for b in range(3):
            cells, origin = grids[b][0], grids[b][1]
            goal = tuple(batch.goal_cells((origin, RES, nx, ny), goals[b:b + 1])[0].tolist())
            r = PC.plan(cells, origin, RES, moved[b, :2], goal, LETHAL, CAP, GAIN, 15)
            got = (int(status[b]), int(poses[b]), tuple(cell[b].tolist()), int(dist[b]))
            assert got == (r["status"], r["poses"], tuple(r["start"]), r["dist"]), (b, got, r["status"], r["poses"], r["start"], r["dist"])
            seen.add(r["status"])
            if r["field"] is not None:
                assert same(bat.resident_read_plan_field(b, (ny, nx)), r["field"]), b
            x, y = bat.resident_read_path(b)
            want = r["path"] if r["path"] is not None else lines[b]
            assert same(x, want[0]) and same(y, want[1]), b
            differs += r["dist"] != PR.plan(cells, origin, RES, moved[b, :2], goal, LETHAL, CAP)["dist"]
        assert PR.OK in seen and differs >= 1, (seen, differs)
    finally:
        BS.close_all(bat, tw)


# 7. the closed loop ------------------------------------------------------------------------------------------------------------------
def test_twenty_ticks_of_a_fleet_that_plans_with_penalties_equal_a_twin_that_plans_on_the_host():
    """Two robots discover a wall with their simulated sensors; every tick their maps follow them, and every fifth they replan
    with penalties to a world goal behind the wall's gap.  The twin reads its poses and cells back, decides the follow and runs
    the checker, and installs the result with _resident_set_paths.  It runs first and counts, on its own read-backs, how many of
    its plans differ from the unweighted plan of the same inputs."""
    p = configs.diff_drive_defaults(256, 15)
    nx, ny, cap, ticks = 48, 40, 96, 20
    world, wo = walled_world()
    starts = [(40, 40), (42, 31)]
    anchors = [(c[0] - nx // 2, c[1] - ny // 2) for c in starts]
    origins = [(wo[0] + a[0] * RES, wo[1] + a[1] * RES) for a in anchors]
    s0 = np.zeros((2, 3))
    s0[:, :2] = [pose_at(c, origin=wo) for c in starts]
    seeds = np.array([BS.instance_seed(0), BS.instance_seed(1)], dtype=np.uint64)
    line = [(s0[b, 0] + RES * np.arange(200.0), np.full(200, s0[b, 1])) for b in range(2)]
    infl = batch.inflation_profile(0.75, RES)
    beams = batch.beam_fan(120, 24)
    goals = [np.array([[wo[0] + 62.5 * RES, wo[1] + 37.5 * RES], [wo[0] + 62.5 * RES, wo[1] + 38.5 * RES]]),
             np.array([[wo[0] + 60.5 * RES, wo[1] + 44.5 * RES], [wo[0] + 60.5 * RES, wo[1] + 30.5 * RES]])]

    def make():
        bat = BatchController(p, 2)
        bat.resident_set_paths(line, RES)
        bat.resident_set_poses(s0, seeds)
        bat.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), o, RES, 0.0, 128) for o in origins], infl, [0, 1], 5.0)
        bat.set_world(world, 128, wo, RES, anchors, len(beams))
        return bat

    def leaves(bat):
        out = [bat.resident_read_trace(b).tobytes() for b in range(2)] + CS.tick_bits(bat)
        out += [a.tobytes() for a in bat.resident_read()[:5]]
        out += [np.concatenate(bat.resident_read_path(b)).tobytes() for b in range(2)]
        out += [bat.read_occupancy(m).tobytes() + CS.derived(bat, m).tobytes() for m in range(2)]
        return out + [repr(bat.get_occupancy())]

    tw = make()
    twin = Twin(tw, origins, nx, ny)
    tw.roll_occupancy([0, 1], 0, 0)
    paths, plans, differs, log = [(x.copy(), y.copy()) for x, y in line], 0, 0, []
    for t in range(ticks):
        tw.resident_step_enqueue(p.dt, t)
        twin.follow([0, 1], 2, 3)
        tw.resident_sense([0, 1], beams)
        if t % 5 == 4:
            st = tw.resident_read()[0]
            grids = tw.get_grids()[0]
            for b in range(2):
                cells, origin = grids[b][0], grids[b][1]
                goal = tuple(batch.goal_cells((origin, RES, nx, ny), goals[(t // 5) % 2][b:b + 1])[0].tolist())
                r = PC.plan(cells, origin, RES, st[b, :2], goal, LETHAL, cap, GAIN, 15)
                log.append((r["status"], r["poses"], tuple(r["start"]), r["dist"]))
                if r["path"] is not None:
                    paths[b] = r["path"]
                    plans += 1
                    u = PR.plan(cells, origin, RES, st[b, :2], goal, LETHAL, cap)
                    differs += not (same(u["path"][0], r["path"][0]) and same(u["path"][1], r["path"][1]))
            tw.resident_set_paths(paths, RES)
    print("plans:", plans, "of them unlike the unweighted plan:", differs, "rows:", log, "offsets:", twin.c.tolist())
    assert plans >= 6 and 3 * differs >= plans, (plans, differs, log)
    want = leaves(tw)
    # the planning fleet: nothing is read until the last tick has been enqueued
    bat = make()
    try:
        bat.resident_set_plan(cap, False)
        bat.resident_set_plan_penalty(GAIN, 15)
        bat.resident_set_follow(True)
        for t in range(ticks):
            bat.resident_step_enqueue(p.dt, t)
            bat.resident_follow([0, 1], 2, 3)
            bat.resident_sense([0, 1], beams)
            if t % 5 == 4:
                bat.resident_plan_goals([0, 1], goals[(t // 5) % 2], LETHAL, nx * ny + 1)
        status, poses, cell, dist, _ = bat.resident_read_plan()
        assert [(status[b], poses[b], tuple(cell[b]), dist[b]) for b in range(2)] == log[-2:]
        got = leaves(bat)
        assert len(got) == len(want)
        assert [i for i, (x, y) in enumerate(zip(got, want)) if x != y] == []
    finally:
        BS.close_all(bat, tw)

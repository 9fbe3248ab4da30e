"""GPU tests (-m gpu) of the batch handles' device planner (ccv_mppi_batch_resident_set_plan, _plan_enqueue and their companions;
BatchController.resident_plan).

The contract is in integers but for one pose-to-cell and one cell-to-pose step, and the field is the one fixpoint of its
relaxation whatever the device's order, so everything -- field, status, L, D(start), start cell and every bit of the path -- is
held against tests/plan_reference.py with no tolerance; only `sweeps` is the device's own, held inside [1, J].  The maps have a
resolution of 2^-2 and origins that are multiples of it, so that a pose can be put exactly on a cell edge.  ccv_mppi_batch_set_grids
refuses cells that are not finite, so a NaN cell cannot reach the device through it: NaN is the checker's own test
(tests/test_plan_reference.py), the cells at `lethal` and one ulp above it are here.  No test asserts a time, looks into a kernel's
assembly, or checks from the host that the call did not synchronise.
"""
import ctypes as C

import numpy as np
import pytest

import batch_support as BS
import costmap_support as CS
import plan_reference as PR
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import same
from oracle import oracle_lib as O

pytestmark = pytest.mark.gpu
i32p = C.POINTER(C.c_int32)
ORIGIN, RES, LETHAL = PR.ORIGIN, PR.RES, PR.LETHAL
B = 8
CAP = 1024


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.fixture(scope="module")
def fleet():
    bat = BatchController(configs.diff_drive_defaults(128, 15), B)
    yield bat
    bat.close()


def pose_at(cell, frac=(0.5, 0.5)):
    return (ORIGIN[0] + (cell[0] + frac[0]) * RES, ORIGIN[1] + (cell[1] + frac[1]) * RES)


def line_paths(n=(5, 9, 3, 7, 4, 6, 8, 2)):
    """B short straight paths of different lengths: what the instances track before they plan"""
    return [(ORIGIN[0] + RES * np.arange(k, dtype=np.float64), np.full(k, ORIGIN[1] + 0.1 * b)) for b, k in enumerate(n)]


def install(bat, maps, map_of, poses, capacity=CAP, keep=True, paths=None):
    """maps: float cells per map; every instance on map_of[b]; planning set; returns the paths the instances start with"""
    paths = line_paths() if paths is None else paths
    bat.resident_set_paths(paths, RES)
    st = np.zeros((bat.B, 3))
    st[:len(poses), :2] = np.asarray(poses, dtype=np.float64)
    bat.resident_set_poses(st, np.arange(1, bat.B + 1, dtype=np.uint64))
    bat.set_grids([(m, ORIGIN, RES, 0.0) for m in maps], np.asarray(map_of, dtype=np.int32), 1.0)
    bat.resident_set_plan(capacity, keep)
    return [(np.array(x), np.array(y)) for x, y in paths]


def expect(maps, map_of, poses, goals, instances, capacity, converged=True):
    cap = np.broadcast_to(np.asarray(capacity), (B,))
    return {b: PR.plan(maps[map_of[b]], ORIGIN, RES, poses[b], g, LETHAL, int(cap[b]), converged=converged) for b, g in zip(instances, goals)}


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
            assert same(bat.resident_read_plan_field(b, (ny, nx)), r["field"]), b
            assert 1 <= sweeps[b] <= nx * ny + 1 and (jacobi is None or sweeps[b] <= jacobi[b]), (b, sweeps[b])
        elif r["status"] != PR.NOT_CONVERGED:
            assert sweeps[b] == 0
    for b in range(bat.B):
        x, y = bat.resident_read_path(b)
        assert same(x, paths[b][0]) and same(y, paths[b][1]), (b, len(x), len(paths[b][0]))


def raw_plan(bat, instances, goals, lethal=LETHAL, max_sweeps=PR.MAX_FIELD, want=capi.OK):
    inst = np.array(instances, dtype=np.int32)
    g = np.array(goals, dtype=np.int32).reshape(-1, 2).copy()
    rc = bat.lib.ccv_mppi_batch_resident_plan_enqueue(bat._h, len(inst), inst.ctypes.data_as(i32p), g.ctypes.data_as(i32p), float(lethal), int(max_sweeps))
    assert rc == want, (rc, bat.lib.ccv_mppi_batch_last_error(bat._h))
    inst[...] = -5      # (the arrays may be reused when the call returns)
    g[...] = 12345


# 1. from scratch ---------------------------------------------------------------------------------------------------------------------
# the issue's sizes; the kernel's own edges: a pitch nx + 1 of every residue mod 4 (it is padded to 2 mod 4), rows + columns one below,
# at and one above the workgroup's 1024 threads (a thread then owns two strips), and the largest images -- a wide one, whose pitch
# cannot be padded, and a single row of 27 304 cells
SHAPES = ((1, 1), (2, 2), (1, 200), (200, 1), (67, 45), (130, 70), (256, 256), (284, 284),
          (3, 2), (4, 3), (5, 2), (6, 3), (1, 1022), (1023, 1), (2, 1023), (318, 254), (27304, 1))
BIG = 20000   # cells: above it two kinds per size, so that the checker's own time stays small


def kinds_of(nx, ny):
    if nx * ny <= BIG:
        return PR.KINDS
    return {(256, 256): ("serpentine", "random"), (284, 284): ("empty", "wall_with_gap")}.get((nx, ny), ("empty",))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_a_plan_equals_the_checker_from_scratch(fleet, nx, ny):
    """up to six instances on maps of their own kind plan in one call, each from near cell (0, 0) to near the far corner"""
    kinds = kinds_of(nx, ny)
    cases = [PR.case(k, nx, ny, seed=nx + 3 * ny, finite=True) for k in kinds]
    maps, n = [c[0] for c in cases], len(cases)
    # ... and one more on the first map, from the free cell nearest to three quarters of the way
    map_of = list(range(n)) + [0] + [-1] * (B - n - 1)
    poses = [pose_at(c[1], (0.25, 0.75)) for c in cases] + [pose_at(PR.free_cell(maps[0], LETHAL, (3 * nx // 4, 3 * ny // 4)), (0.5, 0.0))] * (B - n)
    goals = [c[2] for c in cases] + [cases[0][2]]
    paths = install(fleet, maps, map_of, poses)
    fleet.resident_plan(list(range(n + 1)), goals, LETHAL)
    want = expect(maps, map_of, poses, goals, range(n + 1), CAP)
    holds(fleet, want, paths, maps, map_of)
    seen = {want[b]["status"] for b in want}
    if nx * ny > 4 and len(kinds) == len(PR.KINDS):
        assert PR.UNREACHABLE in seen and (PR.OK in seen or PR.TRUNCATED in seen), seen
    if (nx, ny) == (256, 256):
        assert want[0]["status"] == PR.UNREACHABLE and want[0]["dist"] == PR.FAR and (want[0]["field"] == PR.FAR).sum() > 10000


def test_a_map_above_the_size_limit_is_refused(fleet):
    maps = [PR.empty(285, 285), PR.empty(284, 284)]
    paths = install(fleet, maps, [0, 1] + [-1] * 6, [pose_at((0, 0))] * 2)
    raw_plan(fleet, [0], [(3, 3)], want=capi.ERR_INVALID_ARG)
    raw_plan(fleet, [1, 0], [(3, 3), (3, 3)], want=capi.ERR_INVALID_ARG)
    status = fleet.resident_read_plan()[0]
    assert (status == 0).all()
    holds(fleet, {}, paths, maps, [0, 1])
    raw_plan(fleet, [1], [(3, 3)])
    assert fleet.resident_read_plan()[0][1] == PR.OK


# 2. starts, capacities, sweeps, entries ---------------------------------------------------------------------------------------------------
def test_starts_on_an_edge_outside_nan_blocked_and_on_the_goal(fleet):
    cells, start, goal = PR.case("random", 67, 45, seed=5, finite=True)
    wall = tuple(np.argwhere(PR.blocked(cells, LETHAL))[7][::-1].tolist())
    reached = PR.field_dijkstra(cells, goal, LETHAL) < PR.FAR
    at_lethal = tuple(np.argwhere((cells == LETHAL) & reached)[3][::-1].tolist())
    poses = [pose_at(start, (0.0, 0.0)),                                    # exactly on the cell's lower edges
             (np.nextafter(pose_at(start)[0] + RES / 2, -np.inf), pose_at(start, (0.0, 0.999))[1]),   # the last doubles of the cell
             (ORIGIN[0] - 1e-9, ORIGIN[1] + 1.0),                           # just outside
             (ORIGIN[0] + 67 * RES, ORIGIN[1] + 1.0),                       # at nx: outside
             (np.nan, ORIGIN[1] + 1.0), pose_at(wall), pose_at(goal, (0.9, 0.1)), pose_at(at_lethal)]
    maps, map_of = [cells], [0] * B
    paths = install(fleet, maps, map_of, poses)
    goals = [goal] * B
    fleet.resident_plan(list(range(B)), goals, LETHAL)
    want = expect(maps, map_of, poses, goals, range(B), CAP)
    assert [want[b]["status"] for b in range(B)] == [PR.OK, PR.OK, PR.NO_START, PR.NO_START, PR.NO_START, PR.START_BLOCKED, PR.OK, PR.OK]
    assert want[0]["start"] == start and want[1]["start"] == start and want[6]["poses"] == 1 and want[6]["dist"] == 0
    holds(fleet, want, paths, maps, map_of)
    # a blocked goal, and a cell one ulp above lethal as the goal
    above = tuple(np.argwhere(cells == np.nextafter(LETHAL, np.float32(np.inf)))[0][::-1].tolist())
    fleet.resident_plan([0, 1, 7], [wall, above, at_lethal], LETHAL)
    want = expect(maps, map_of, poses, [wall, above, at_lethal], [0, 1, 7], CAP)
    assert [want[b]["status"] for b in (0, 1, 7)] == [PR.GOAL_BLOCKED, PR.GOAL_BLOCKED, PR.OK] and want[7]["poses"] == 1
    holds(fleet, want, paths, maps, map_of)


def test_capacity_l_l_minus_one_and_one(fleet):
    cells, start, goal = PR.case("wall_with_gap", 67, 45, finite=True)
    L = PR.plan(cells, ORIGIN, RES, pose_at(start), goal, LETHAL, PR.MAX_POSES)["poses"]
    assert L > 60
    cap = np.array([L, L - 1, 1, L + 1, 0, PR.MAX_POSES, 2, 1], dtype=np.int32)
    maps, map_of, poses = [cells], [0] * B, [pose_at(start)] * B
    paths = install(fleet, maps, map_of, poses, capacity=cap)
    assert same(fleet.resident_get_plan()[0], cap) and fleet.resident_get_plan()[1] is True
    named = [0, 1, 2, 3, 5, 6, 7]
    fleet.resident_plan(named, [goal] * 7, LETHAL)
    want = expect(maps, map_of, poses, [goal] * 7, named, cap)
    assert [want[b]["status"] for b in named] == [PR.OK, PR.TRUNCATED, PR.TRUNCATED, PR.OK, PR.OK, PR.TRUNCATED, PR.TRUNCATED]
    assert [len(want[b]["path"][0]) for b in named] == [L, L - 1, 1, L, L, 2, 1] and all(want[b]["poses"] == L for b in named)
    holds(fleet, want, paths, maps, map_of)
    raw_plan(fleet, [4], [goal], want=capi.ERR_INVALID_ARG)   # (capacity 0)


def test_max_sweeps_j_converges_and_one_does_not(fleet):
    kinds = ("empty", "random", "wall_with_gap", "serpentine")
    cases = [PR.case(k, 23, 17, seed=2, finite=True) for k in kinds]
    maps, map_of = [c[0] for c in cases], [0, 1, 2, 3, 0, 1, 2, 3]
    poses = [pose_at(cases[m][1]) for m in map_of]
    goals = [cases[m][2] for m in map_of]
    J = [PR.field_jacobi(maps[m], goals[b], LETHAL)[1] for b, m in enumerate(map_of)]
    assert max(J) > 40 and min(J) > 2
    paths = install(fleet, maps, map_of, poses)
    for b in range(4):   # one call per J: max_sweeps is the call's
        raw_plan(fleet, [b], [goals[b]], max_sweeps=J[b])
    want = expect(maps, map_of, poses, goals[:4], range(4), CAP)
    assert all(want[b]["status"] in (PR.OK, PR.UNREACHABLE) for b in range(4))
    holds(fleet, want, paths, maps, map_of, jacobi=J)
    # one sweep: the goal's free neighbour falls in it, so no sweep is without a change -- and no bit changes
    before = [fleet.resident_read_plan_field(b, maps[map_of[b]].shape).tobytes() for b in range(4)]
    raw_plan(fleet, [4, 5, 6, 7, 0], goals[4:] + [goals[0]], max_sweeps=1)
    want = expect(maps, map_of, poses, goals[4:] + [goals[0]], [4, 5, 6, 7, 0], CAP, converged=False)
    holds(fleet, want, paths, maps, map_of)
    status, _, _, _, sweeps = fleet.resident_read_plan()
    assert (status[[4, 5, 6, 7, 0]] == PR.NOT_CONVERGED).all() and (sweeps[[4, 5, 6, 7, 0]] == 1).all()
    assert fleet.lib.ccv_mppi_batch_resident_read_plan_field(fleet._h, 0, np.zeros(23 * 17, dtype=np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))) == capi.ERR_STATE
    raw_plan(fleet, [1], [goals[1]], max_sweeps=J[1])
    assert fleet.resident_read_plan_field(1, maps[1].shape).tobytes() == before[1]


@pytest.mark.parametrize("keep", (True, False))
def test_one_entry_b_entries_reversed_and_two_instances_on_one_map(fleet, keep):
    cases = [PR.case(k, 31, 19, seed=9, finite=True) for k in ("random", "wall_with_gap", "diagonal_pair")]
    maps, map_of = [c[0] for c in cases], [0, 1, 2, 0, 1, 2, 0, 0]
    starts = [PR.free_cell(maps[m], LETHAL, (3 * b, b)) for b, m in enumerate(map_of)]
    poses = [pose_at(s, (0.1 * b, 0.9 - 0.1 * b)) for b, s in enumerate(starts)]
    goals = [cases[m][2] for m in map_of]
    paths = install(fleet, maps, map_of, poses, keep=keep)
    reads = []
    for named in ([3], list(range(B)), list(range(B))[::-1], [6, 0, 7]):
        g = [goals[b] if len(named) > 3 else starts[(b + 1) % B] for b in named]
        raw_plan(fleet, named, g)
        want = expect(maps, map_of, poses, g, named, CAP)
        if not keep:
            for r in want.values():
                r["field"] = None
        status, n_poses, cell, dist, sweeps = fleet.resident_read_plan()
        for b, r in want.items():
            assert (status[b], n_poses[b], tuple(cell[b]), dist[b]) == (r["status"], r["poses"], tuple(r["start"]), r["dist"]), b
            if r["path"] is not None:
                paths[b] = r["path"]
        if keep:
            holds(fleet, want, paths, maps, map_of)
        reads.append([tuple(a.tobytes() for a in fleet.resident_read_path(b)) for b in range(B)])
        assert all(same(fleet.resident_read_path(b)[0], paths[b][0]) and same(fleet.resident_read_path(b)[1], paths[b][1]) for b in range(B))
    if not keep:
        out = np.zeros(31 * 19, dtype=np.uint16)
        assert fleet.lib.ccv_mppi_batch_resident_read_plan_field(fleet._h, 0, out.ctypes.data_as(C.POINTER(C.c_uint16))) == capi.ERR_STATE
    assert reads[1] == reads[2]   # (the entries reversed: the same paths)


# 3. plumbing ----------------------------------------------------------------------------------------------------------------------------
def scene():
    p = configs.diff_drive_defaults(256, 15)
    cells, start, goal = PR.case("wall_with_gap", 41, 29, finite=True)
    maps = [cells, PR.case("random", 41, 29, seed=4, finite=True)[0]]
    map_of = [0, 1, 0, -1]
    starts = [start, PR.free_cell(maps[1], LETHAL, (2, 2)), PR.free_cell(cells, LETHAL, (5, 20)), (1, 1)]
    s0 = np.zeros((4, 3))
    s0[:, :2] = [pose_at(s) for s in starts]
    goals = [goal, PR.case("random", 41, 29, seed=4, finite=True)[2], goal]
    return p, maps, map_of, s0, np.arange(11, 15, dtype=np.uint64), goals


def tick(bat, p, s0, seeds, it=0):
    bat.resident_set_poses(s0, seeds)
    bat.set_nominal(np.zeros((bat.B, p.horizon - 1, p.udim)))
    bat.resident_step_enqueue(p.dt, it, advance=False)
    return CS.tick_bits(bat) + [a.tobytes() for a in bat.resident_read()[2:4]]


def state(bat, shapes):
    out = [a.tobytes() for a in bat.resident_read_plan()]
    out += [a.tobytes() for b in range(bat.B) for a in bat.resident_read_path(b)]
    status = bat.resident_read_plan()[0]
    return out + [bat.resident_read_plan_field(b, shapes[b]).tobytes() for b in range(bat.B) if status[b] in (1, 2, 6)]


def test_refusals_setters_and_what_keeps_a_planned_path():
    p, maps, map_of, s0, seeds, goals = scene()
    bat = BatchController(p, 4)
    lib, ip = bat.lib, lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(i32p)
    shapes = [maps[max(m, 0)].shape for m in map_of]
    # before anything is set
    assert lib.ccv_mppi_batch_resident_set_plan(bat._h, ip([8] * 4), 1) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_resident_get_plan(bat._h, None, None) == capi.ERR_STATE
    paths = [(ORIGIN[0] + RES * np.arange(6.0 + b), np.full(6 + b, ORIGIN[1] + 2.0 + b)) for b in range(4)]
    bat.resident_set_paths(paths, [RES, RES, RES * 2, RES])
    raw_plan(bat, [0], [goals[0]], want=capi.ERR_STATE)   # (planning not set)
    bits0 = None
    assert lib.ccv_mppi_batch_resident_set_plan(bat._h, ip([8, -1, 8, 8]), 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_set_plan(bat._h, ip([8, capi.PLAN_MAX_POSES + 1, 8, 8]), 1) == capi.ERR_INVALID_ARG
    bat.resident_set_plan([200, 200, 200, 0], True)
    raw_plan(bat, [0], [goals[0]], want=capi.ERR_STATE)   # (no resident poses)
    bat.set_grids([(m, ORIGIN, RES, 0.0) for m in maps], np.asarray(map_of, dtype=np.int32), 1.0)
    bits0 = tick(bat, p, s0, seeds)
    raw_plan(bat, [0, 1], goals[:2])
    before, bits = state(bat, shapes), tick(bat, p, s0, seeds)
    assert bits != bits0 and bat.resident_read_plan()[0].tolist() == [1, 1, 0, 0]
    # every refusal of the call: nothing changes
    for inst, g, lethal, sweeps in (([], [], LETHAL, 9), ([0, 1, 2, 3, 0], [goals[0]] * 5, LETHAL, 9), ([4], [goals[0]], LETHAL, 9), ([-1], [goals[0]], LETHAL, 9),
                                    ([0, 0], [goals[0]] * 2, LETHAL, 9), ([3], [goals[0]], LETHAL, 9), ([1, 3], goals[:2], LETHAL, 9),
                                    ([0], [(41, 3)], LETHAL, 9), ([0], [(3, 29)], LETHAL, 9), ([0], [(-1, 3)], LETHAL, 9), ([1, 0], [goals[1], (3, -1)], LETHAL, 9),
                                    ([2], [goals[2]], LETHAL, 9),   # (its path's resolution is not its map's)
                                    ([0], [goals[0]], np.nan, 9), ([0], [goals[0]], LETHAL, 0), ([0], [goals[0]], LETHAL, -3),
                                    ([0], [goals[0]], LETHAL, capi.PLAN_MAX_FIELD + 1)):
        raw_plan(bat, inst, g, lethal, sweeps, want=capi.ERR_INVALID_ARG)
    call = lib.ccv_mppi_batch_resident_plan_enqueue
    assert call(bat._h, 1, None, ip(goals[0]), 0.5, 9) == capi.ERR_INVALID_ARG and call(bat._h, 1, ip([0]), None, 0.5, 9) == capi.ERR_INVALID_ARG
    out = np.zeros(41 * 29, dtype=np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))
    assert lib.ccv_mppi_batch_resident_read_plan_field(bat._h, 4, out) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_plan_field(bat._h, 2, out) == capi.ERR_STATE     # (never planned)
    assert lib.ccv_mppi_batch_resident_read_plan_field(bat._h, 3, out) == capi.ERR_STATE     # (capacity 0)
    assert lib.ccv_mppi_batch_resident_read_plan_field(bat._h, 0, None) == capi.ERR_INVALID_ARG
    assert state(bat, shapes) == before and tick(bat, p, s0, seeds) == bits
    # _set_poses keeps a planned path (tick() calls it); so does a second _set_plan, which lays the paths out again
    planned = [bat.resident_read_path(b) for b in range(4)]
    assert len(planned[0][0]) > 30 and len(planned[2][0]) == 8
    bat.resident_set_plan([300, 64, 0, 5], False)
    assert all(same(bat.resident_read_path(b)[k], planned[b][k]) for b in range(4) for k in (0, 1))
    assert tick(bat, p, s0, seeds) == bits and bat.resident_read_plan()[0].tolist() == [0, 0, 0, 0]
    raw_plan(bat, [1], [goals[1]])   # (capacity 64 now: the longer path of the first plan stays where the new one is shorter)
    r = PR.plan(maps[1], ORIGIN, RES, s0[1, :2], goals[1], LETHAL, 64)
    assert same(bat.resident_read_path(1)[0], r["path"][0]) and bat.resident_read_plan()[0][1] == r["status"]
    # planning off keeps the paths; the host knows their lengths again
    bat.resident_set_plan(None)
    assert lib.ccv_mppi_batch_resident_get_plan(bat._h, None, None) == capi.ERR_STATE
    raw_plan(bat, [0], [goals[0]], want=capi.ERR_STATE)
    kept = [bat.resident_read_path(b) for b in range(4)]
    assert same(kept[0][0], planned[0][0]) and same(kept[1][1], r["path"][1])
    bat.resident_set_poses(s0, seeds)
    assert all(same(bat.resident_read_path(b)[k], kept[b][k]) for b in range(4) for k in (0, 1))
    # _set_paths drops planning
    bat.resident_set_plan(16, True)
    bat.resident_set_paths(paths, [RES, RES, RES * 2, RES])
    assert lib.ccv_mppi_batch_resident_get_plan(bat._h, None, None) == capi.ERR_STATE
    assert all(same(bat.resident_read_path(b)[k], paths[b][k]) for b in range(4) for k in (0, 1))
    assert tick(bat, p, s0, seeds) == bits0
    bat.close()


def test_one_instances_plan_changes_no_bit_of_another_instance():
    p, maps, map_of, s0, seeds, goals = scene()
    snaps = []
    for planned in (False, True):
        bat = BatchController(p, 4)
        bat.resident_set_paths([(ORIGIN[0] + RES * np.arange(6.0 + b), np.full(6 + b, ORIGIN[1] + 2.0 + b)) for b in range(4)], RES)
        bat.set_grids([(m, ORIGIN, RES, 0.0) for m in maps], np.asarray(map_of, dtype=np.int32), 1.0)
        bat.resident_set_plan(200, True)
        bat.resident_set_poses(s0, seeds)
        if planned:
            bat.resident_plan([2], [goals[2]], LETHAL)   # (instance 0 shares its map)
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        snaps.append([(bat.get_nominal()[b].tobytes(), bat.read_costs(b).tobytes(), bat.read_weights(b).tobytes(), bat.read_candidates(b).tobytes(),
                       bat.resident_read()[2][b].tobytes()) + tuple(a.tobytes() for a in bat.resident_read_path(b)) for b in range(4)] +
                     [bat.resident_read_plan()[0].tolist()])
        bat.close()
    assert snaps[0][2] != snaps[1][2] and snaps[1][4] == [0, 0, 1, 0]
    assert [snaps[0][b] == snaps[1][b] for b in (0, 1, 3)] == [True] * 3


def test_planning_returns_all_device_and_pinned_memory():
    import torch
    p = configs.diff_drive_defaults(256, 15)
    cells = PR.wall_with_gap(200, 150)
    s0 = np.zeros((16, 3))
    s0[:, :2] = pose_at((1, 1))

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        bat = BatchController(p, 16)
        bat.resident_set_paths(line_paths()[0], RES)
        bat.resident_set_poses(s0, 1)
        bat.set_grids([(cells, ORIGIN, RES, 0.0)], np.zeros(16, dtype=np.int32), 1.0)
        bat.resident_set_plan(capi.PLAN_MAX_POSES, True)      # (creates the staging ring: no occupancy is set)
        for _ in range(capi.OCC_PATCH_SLOTS + 1):
            bat.resident_plan([0, 5], [(190, 140), (3, 140)], LETHAL)
        bat.resident_set_plan(512, False)                     # (a new layout takes the old one's place)
        bat.resident_plan([7], [(190, 140)], LETHAL)
        bat.resident_set_plan(None)
        bat.resident_set_plan(capi.PLAN_MAX_POSES, True)
        bat.resident_set_paths(line_paths()[1], RES)          # (drops planning)
        bat.resident_set_plan(capi.PLAN_MAX_POSES, True)
        bat.close()                                           # (... and so does destroy)

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)


# 4. a planning fleet against a twin that plans on the host ------------------------------------------------------------------------------
def test_thirty_ticks_of_a_planning_fleet_equal_a_twin_that_plans_on_the_host():
    """Two robots discover a wall with their simulated sensors and replan every fifth tick, to a goal that alternates between two
    corners; their maps roll once on the way.  The twin makes the same calls but for the plans: it reads its poses and cells back,
    runs the checker and installs the result with _resident_set_paths.  It runs first, and counts on its own read-backs how many
    plans changed the next tick's window: the window it read against ccv_mppi_calc_ref_path over the path before the plan."""
    p = configs.diff_drive_defaults(256, 15)
    nx, ny, cap, ticks = 64, 48, 96, 30
    world = np.zeros((70, 100), dtype=np.uint8)
    world[0:44, 22] = 255
    world[8:12, 22] = 0          # (a gap low in the wall; the straight paths run into the wall above it)
    starts = [(5, 20), (7, 29)]
    s0 = np.zeros((2, 3))
    s0[:, :2] = [pose_at(s) for s in starts]
    seeds = np.array([BS.instance_seed(0), BS.instance_seed(1)], dtype=np.uint64)
    line = [(s0[b, 0] + RES * np.arange(200.0), np.full(200, s0[b, 1])) for b in range(2)]
    infl = batch.inflation_profile(0.75, RES)
    beams = batch.beam_fan(120, 24)
    corners = [np.array([[ORIGIN[0] + 15.0, ORIGIN[1] + 1.0]] * 2), np.array([[ORIGIN[0] + 15.2, ORIGIN[1] + 10.6]] * 2)]
    roll_at, roll_by = 12, (3, 2)

    def make():
        bat = BatchController(p, 2)
        bat.resident_set_paths(line, RES)
        bat.resident_set_poses(s0, seeds)
        bat.set_occupancy([(np.zeros((ny, nx), dtype=np.uint8), ORIGIN, RES, 0.0, 128)] * 2, infl, [0, 1], 5.0)
        bat.set_world(world, 128, ORIGIN, RES, [(0, 0), (0, 0)], len(beams))
        bat.roll_occupancy([0, 1], 0, 0)   # (primes the second set of layers: the later roll allocates nothing)
        return bat

    def origin_at(t):
        c = (roll_by[0], roll_by[1]) if t >= roll_at else (0, 0)
        return (ORIGIN[0] + float(c[0]) * RES, ORIGIN[1] + float(c[1]) * RES)

    def after_tick(bat, t):
        bat.resident_sense([0, 1], beams)
        if t == roll_at:
            bat.roll_occupancy([0, 1], roll_by[0], roll_by[1])

    def goals_at(t, k):
        return batch.goal_cells((origin_at(t), RES, nx, ny), corners[k % 2])

    # the twin
    twin, paths, plans, changed, log = make(), [(x.copy(), y.copy()) for x, y in line], 0, 0, []
    pending = None
    for t in range(ticks):
        twin.resident_step_enqueue(p.dt, t)
        if pending is not None:   # the tick after a plan: did its window change?
            st, _, xr, yr, _, _ = twin.resident_read()
            for b, old in pending:
                _, cx, cy, _ = O.calc_ref_path(old[0], old[1], st[b, 0], st[b, 1], p.v_ref, p.dt, RES, p.horizon)
                changed += not (np.asarray(cx).tobytes() == xr[b].tobytes() and np.asarray(cy).tobytes() == yr[b].tobytes())
            pending = None
        after_tick(twin, t)
        if t % 5 == 4:
            st = twin.resident_read()[0]
            maps = twin.get_grids()[0]
            goals = goals_at(t, t // 5)
            pending = []
            for b in range(2):
                cells, origin = maps[b][0], maps[b][1]
                assert tuple(origin) == origin_at(t)
                r = PR.plan(cells, origin, RES, st[b, :2], goals[b], LETHAL, cap)
                log.append((r["status"], r["poses"], tuple(r["start"]), r["dist"]))
                if r["path"] is not None:
                    pending.append((b, paths[b]))
                    paths[b] = r["path"]
                    plans += 1
            twin.resident_set_paths(paths, RES)
    assert plans >= 8 and 3 * changed >= plans, (plans, changed, log)
    assert any(PR.blocked(m[0], LETHAL).any() for m in twin.get_grids()[0])   # (the wall was seen)
    # the planning fleet: nothing is read until the last tick has been enqueued
    fleet2 = make()
    fleet2.resident_set_plan(cap, False)
    for t in range(ticks):
        fleet2.resident_step_enqueue(p.dt, t)
        after_tick(fleet2, t)
        if t % 5 == 4:
            fleet2.resident_plan([0, 1], goals_at(t, t // 5), LETHAL)
    status, poses, cell, dist, _ = fleet2.resident_read_plan()
    assert [(status[b], poses[b], tuple(cell[b]), dist[b]) for b in range(2)] == log[-2:]
    for b in range(2):
        assert same(fleet2.resident_read_trace(b), twin.resident_read_trace(b)), b
        assert all(same(a, c) for a, c in zip(fleet2.resident_read_path(b), paths[b])), b
        assert all(same(a, c) for a, c in zip(fleet2.resident_read_path(b), twin.resident_read_path(b))), b
    assert CS.tick_bits(fleet2) == CS.tick_bits(twin)
    assert all(same(a, c) for a, c in zip(fleet2.resident_read()[:5], twin.resident_read()[:5]))
    BS.close_all(fleet2, twin)

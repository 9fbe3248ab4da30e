"""CPU tests of tests/plan_reference.py, the checker of the device planner: its three ways to the
distance field agree, every deliberately wrong version is told apart by one of the listed cases, the field saturates where the
spec says it does, and the two floating-point steps behave at their edges.  Nothing here touches the library."""
import itertools

import numpy as np
import pytest

import plan_reference as PR


def test_dijkstra_jacobi_and_bellman_ford_agree_on_small_maps():
    for (nx, ny), kind in itertools.product(PR.SMALL_SHAPES, PR.KINDS):
        cells, start, goal = PR.case(kind, nx, ny, seed=nx + ny)
        D = PR.field_dijkstra(cells, goal, PR.LETHAL)
        Dj, J = PR.field_jacobi(cells, goal, PR.LETHAL)
        assert D.dtype == np.uint16 and (D == Dj).all() and (D == PR.field_bellman_ford(cells, goal, PR.LETHAL)).all(), (kind, nx, ny)
        assert 1 <= J <= nx * ny + 1
        assert ((D == PR.BLOCKED) == PR.blocked(cells, PR.LETHAL)).all() and D[goal[1], goal[0]] == 0


def test_the_three_agree_on_every_3_by_3_map():
    """all 2^9 patterns of blocked cells, every free goal"""
    for bits in range(512):
        cells = np.array([(bits >> k) & 1 for k in range(9)], dtype=np.float32).reshape(3, 3)
        for gx, gy in itertools.product(range(3), range(3)):
            D = PR.field_dijkstra(cells, (gx, gy), 0.5)
            assert (D == PR.field_jacobi(cells, (gx, gy), 0.5)[0]).all() and (D == PR.field_bellman_ford(cells, (gx, gy), 0.5)).all(), (bits, gx, gy)


def _outcome(cells, pose, goal, capacity, wrong):
    r = PR.plan(cells, PR.ORIGIN, PR.RES, pose, goal, PR.LETHAL, capacity, wrong)
    path = None if r["path"] is None else (r["path"][0].tobytes(), r["path"][1].tobytes())
    return r["status"], r["poses"], r["start"], r["dist"], path, None if r["field"] is None else r["field"].tobytes()


@pytest.mark.parametrize("wrong", PR.WRONG)
def test_every_wrong_version_differs_on_a_listed_case(wrong):
    differs = []
    for (nx, ny), kind in itertools.product(PR.SMALL_SHAPES, PR.KINDS):
        cells, start, goal = PR.case(kind, nx, ny, seed=nx + ny)
        # the pose in the upper right of its cell: rounding moves it
        pose = (PR.ORIGIN[0] + (start[0] + 0.75) * PR.RES, PR.ORIGIN[1] + (start[1] + 0.75) * PR.RES)
        if _outcome(cells, pose, goal, PR.MAX_POSES, wrong) != _outcome(cells, pose, goal, PR.MAX_POSES, None):
            differs.append((kind, nx, ny))
    assert differs, wrong


def test_a_right_version_is_not_told_apart_from_itself():
    cells, start, goal = PR.case("random", 13, 9, seed=3)
    pose = (PR.ORIGIN[0] + (start[0] + 0.5) * PR.RES, PR.ORIGIN[1] + (start[1] + 0.5) * PR.RES)
    assert _outcome(cells, pose, goal, 64, None) == _outcome(cells.copy(), pose, goal, 64, None)


def test_the_256_serpentine_saturates():
    cells = PR.serpentine(256, 256)
    D = PR.field_dijkstra(cells, (0, 254), PR.LETHAL)   # (the far end of the corridor: row 254 is free, its exit at x = 0 ... )
    assert D[0, 0] == PR.FAR and (D == PR.FAR).sum() > 10000 and D[254, 0] == 0
    r = PR.plan(cells, PR.ORIGIN, PR.RES, (PR.ORIGIN[0] + 0.1, PR.ORIGIN[1] + 0.1), (0, 254), PR.LETHAL, 16, field=D)
    assert r["status"] == PR.UNREACHABLE and r["dist"] == PR.FAR and r["path"] is None


def test_a_cell_equal_to_lethal_is_free_and_the_next_float_is_blocked():
    lethal = np.float32(0.3)
    cells = np.array([[lethal, np.nextafter(lethal, np.float32(1)), np.nan, -np.inf, np.inf, np.nextafter(lethal, np.float32(-1))]], dtype=np.float32)
    assert PR.blocked(cells, lethal).tolist() == [[False, True, True, False, True, False]]
    D = PR.field_dijkstra(cells, (0, 0), lethal)
    assert D.tolist() == [[0, PR.BLOCKED, PR.BLOCKED, PR.FAR, PR.BLOCKED, PR.FAR]]


def test_pose_cell_at_its_edges():
    o, r = (-3.0, 1.5), 0.25
    cell = lambda x, y: PR.pose_cell(x, y, o, r, 7, 5)
    assert cell(-3.0, 1.5) == (0, 0) and cell(-2.75, 1.75) == (1, 1)                      # on an edge: the upper cell
    assert cell(np.nextafter(-2.75, -9.0), 1.5) == (0, 0)
    assert cell(np.nextafter(-3.0, -9.0), 1.5) is None and cell(-3.0, np.nextafter(1.5, 0.0)) is None   # just below 0
    assert cell(-3.0 + 7 * r, 1.5) is None and cell(np.nextafter(-3.0 + 7 * r, -9.0), 1.5) == (6, 0)    # at nx
    assert cell(-3.0, 1.5 + 5 * r) is None
    for bad in (np.nan, np.inf, -np.inf):
        assert cell(bad, 1.5) is None and cell(-3.0, bad) is None


def test_descent_order_capacity_and_poses():
    cells = PR.empty(6, 3)
    pose = (PR.ORIGIN[0] + 0.5 * PR.RES, PR.ORIGIN[1] + 0.5 * PR.RES)
    r = PR.plan(cells, PR.ORIGIN, PR.RES, pose, (5, 2), PR.LETHAL, 64)
    # E before NE wherever both descend: three straight moves first, then the two diagonals
    assert r["status"] == PR.OK and r["poses"] == 6 and r["dist"] == 3 * 5 + 2 * 7
    assert r["path"][0].tolist() == [PR.ORIGIN[0] + (x + 0.5) * PR.RES for x in (0, 1, 2, 3, 4, 5)]
    assert r["path"][1].tolist() == [PR.ORIGIN[1] + (y + 0.5) * PR.RES for y in (0, 0, 0, 0, 1, 2)]
    t = PR.plan(cells, PR.ORIGIN, PR.RES, pose, (5, 2), PR.LETHAL, 5)
    assert t["status"] == PR.TRUNCATED and t["poses"] == 6 and len(t["path"][0]) == 5 and t["path"][0].tolist() == r["path"][0][:5].tolist()
    one = PR.plan(cells, PR.ORIGIN, PR.RES, pose, (0, 0), PR.LETHAL, 1)
    assert one["status"] == PR.OK and one["poses"] == 1 and one["dist"] == 0
    # the statuses in their order: no start, start blocked, goal blocked, unreachable
    walls = PR.enclosed(6, 3)
    assert PR.plan(walls, PR.ORIGIN, PR.RES, (np.nan, 0.0), (4, 2), PR.LETHAL, 8)["status"] == PR.NO_START
    inside = (PR.ORIGIN[0] + 4.5 * PR.RES, PR.ORIGIN[1] + 2.5 * PR.RES)
    assert PR.plan(walls, PR.ORIGIN, PR.RES, inside, (4, 2), PR.LETHAL, 8)["status"] == PR.START_BLOCKED
    assert PR.plan(walls, PR.ORIGIN, PR.RES, pose, (4, 2), PR.LETHAL, 8)["status"] == PR.GOAL_BLOCKED
    assert PR.plan(walls, PR.ORIGIN, PR.RES, pose, (5, 2), PR.LETHAL, 8)["status"] == PR.UNREACHABLE
    assert PR.plan(walls, PR.ORIGIN, PR.RES, pose, (5, 2), PR.LETHAL, 8, converged=False)["status"] == PR.NOT_CONVERGED


def test_max_sweeps_one_never_converges_beside_a_free_neighbour():
    D, J = PR.field_jacobi(PR.empty(4, 4), (1, 1), PR.LETHAL, max_sweeps=1)
    assert J == 2 and D[1, 2] == 5

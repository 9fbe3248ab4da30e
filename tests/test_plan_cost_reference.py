"""CPU tests of tests/plan_cost_reference.py, the checker of the weighted device planner: its three ways
to the field agree, gain = 0 and max_penalty = 0 are tests/plan_reference.py in field, route and status, the quantisation behaves
at its edges, the clearance case and the saturating row give the numbers the spec names, every deliberately wrong version is told
apart by a listed case, and what the device quantises with -- plan_multiplier (csrc/mppi_plan_penalty.h), compiled into a
stand-alone host program (tools/plan_penalty_check.cpp) -- and numpy's batch.plan_multiplier equal the checker.  Nothing here
touches the library."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import plan_cost_reference as PC
import plan_reference as PR
from ccv_mppi_path_tracker_amd import batch, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GAIN = 8.0 / float(PR.LETHAL)   # a graded map's products then sit on the integers 0..8 or one float off them


ROUNDS_UP = (f32(float.fromhex("0x1.2a1fd4p-2")), f32(float.fromhex("0x1.b7a7cep+3")))   # (cell, gain): RN(cell * gain) = 4 > cell * gain


def below(v):
    return np.nextafter(f32(v), f32(-np.inf))


# ---- the field three ways ---------------------------------------------------------------------------------------------------------
def test_the_three_agree_on_every_3_by_3_map_with_two_penalty_assignments():
    """all 2^9 patterns of blocked cells, every goal; the free cells graded two ways"""
    grades = [np.array([[0.0, 0.125, 0.25], [0.375, 0.5, 0.0625], [0.45, 0.3, 0.2]], dtype=f32),
              np.array([[0.5, 0.0, 0.5], [0.1, 0.49, 0.26], [0.0, 0.5, 0.13]], dtype=f32)]
    for bits in range(512):
        blocked = np.array([(bits >> k) & 1 for k in range(9)], dtype=bool).reshape(3, 3)
        for k, (grade, gain, maxp) in enumerate(zip(grades, (8.0, 30.0), (15, 6))):
            cells = np.where(blocked, f32(1.0), grade).astype(f32)
            for gx, gy in itertools.product(range(3), range(3)):
                D = PC.field_dijkstra(cells, (gx, gy), 0.5, gain, maxp)
                assert (D == PC.field_jacobi(cells, (gx, gy), 0.5, gain, maxp)[0]).all(), (bits, k, gx, gy)
                if (bits + gx + gy) % 3 == 0:   # (the slow one on a third of them: every pattern with some goal)
                    assert (D == PC.field_bellman_ford(cells, (gx, gy), 0.5, gain, maxp)).all(), (bits, k, gx, gy)


def test_the_three_agree_on_the_listed_maps_with_graded_cells():
    seen = 0
    for (nx, ny), kind in itertools.product(PR.SMALL_SHAPES, PR.KINDS):
        cells, start, goal = PR.case(kind, nx, ny, seed=nx + ny)
        cells = PC.graded(cells, seed=nx)
        assert (PR.blocked(cells, PR.LETHAL) == PR.blocked(PR.case(kind, nx, ny, seed=nx + ny)[0], PR.LETHAL)).all()
        D = PC.field_dijkstra(cells, goal, PR.LETHAL, GAIN, 15)
        Dj, J = PC.field_jacobi(cells, goal, PR.LETHAL, GAIN, 15)
        assert D.dtype == np.uint16 and (D == Dj).all() and (D == PC.field_bellman_ford(cells, goal, PR.LETHAL, GAIN, 15)).all(), (kind, nx, ny)
        assert 1 <= J <= nx * ny + 1
        assert ((D == PR.BLOCKED) == PR.blocked(cells, PR.LETHAL)).all() and D[goal[1], goal[0]] == 0
        seen += int((D != PR.field_dijkstra(cells, goal, PR.LETHAL)).any())
    assert seen > 10   # (the weights matter on these maps)


def test_dijkstra_and_jacobi_agree_on_random_maps():
    rng = np.random.default_rng(7)
    for k in range(300):
        nx, ny = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        cells = (rng.random((ny, nx)) * 0.8).astype(f32)
        cells[rng.random((ny, nx)) < 0.2] = 1.0
        goal = (int(rng.integers(0, nx)), int(rng.integers(0, ny)))
        gain, maxp = float(rng.choice([1.0, 7.5, 20.0, 40.0])), int(rng.integers(1, 16))
        assert (PC.field_dijkstra(cells, goal, 0.75, gain, maxp) == PC.field_jacobi(cells, goal, 0.75, gain, maxp)[0]).all(), k


def _outcome(r):
    path = None if r["path"] is None else (r["path"][0].tobytes(), r["path"][1].tobytes())
    return r["status"], r["poses"], tuple(r["start"]), r["dist"], path, None if r["field"] is None else r["field"].tobytes()


def test_gain_zero_and_max_penalty_zero_are_the_unweighted_plan():
    for (nx, ny), kind in itertools.product(PR.SMALL_SHAPES, PR.KINDS):
        cells, start, goal = PR.case(kind, nx, ny, seed=nx + ny)
        cells = PC.graded(cells, seed=ny)
        pose = (PR.ORIGIN[0] + (start[0] + 0.75) * PR.RES, PR.ORIGIN[1] + (start[1] + 0.75) * PR.RES)
        want = _outcome(PR.plan(cells, PR.ORIGIN, PR.RES, pose, goal, PR.LETHAL, 40))
        for gain, maxp in ((0.0, 15), (GAIN, 0), (0.0, 0), (-0.0, 7)):
            assert _outcome(PC.plan(cells, PR.ORIGIN, PR.RES, pose, goal, PR.LETHAL, 40, gain, maxp)) == want, (kind, nx, ny, gain, maxp)
            assert (PC.field_jacobi(cells, goal, PR.LETHAL, gain, maxp)[0] == PR.field_jacobi(cells, goal, PR.LETHAL)[0]).all()
            assert PC.field_jacobi(cells, goal, PR.LETHAL, gain, maxp)[1] == PR.field_jacobi(cells, goal, PR.LETHAL)[1]
    # the statuses that come before any field
    walls = PR.enclosed(6, 3)
    pose = (PR.ORIGIN[0] + 0.5 * PR.RES, PR.ORIGIN[1] + 0.5 * PR.RES)
    inside = (PR.ORIGIN[0] + 4.5 * PR.RES, PR.ORIGIN[1] + 2.5 * PR.RES)
    for p, g, conv in (((np.nan, 0.0), (4, 2), True), (inside, (4, 2), True), (pose, (4, 2), True), (pose, (5, 2), True), (pose, (5, 2), False)):
        assert _outcome(PC.plan(walls, PR.ORIGIN, PR.RES, p, g, PR.LETHAL, 8, 9.0, 15, converged=conv)) == \
            _outcome(PR.plan(walls, PR.ORIGIN, PR.RES, p, g, PR.LETHAL, 8, converged=conv))


# ---- the quantisation ---------------------------------------------------------------------------------------------------------------
def edge_values():
    """(cell, gain, max_penalty, m) at the edges of the quantisation"""
    tiny = f32(np.nextafter(f32(0), f32(1)))   # the smallest subnormal
    up, up_gain = ROUNDS_UP
    return [
        (f32(0.375), f32(8.0), 15, 4), (below(0.375), f32(8.0), 15, 3),             # the product exactly an integer, and one float below
        (f32(0.5), f32(2.0), 15, 2), (below(0.5), f32(2.0), 15, 1),
        (up, up_gain, 15, 5),                                                       # the fp32 product rounds up to 4: the exact one is below
        (f32(0.5), f32(30.0), 15, 16), (below(0.5), f32(30.0), 15, 15),             # t at max_penalty, and one float below
        (f32(0.5), f32(12.0), 6, 7), (below(0.5), f32(12.0), 6, 6), (f32(0.5), f32(1000.0), 3, 4),
        (f32(0.0), f32(8.0), 15, 1), (f32(-0.0), f32(8.0), 15, 1), (f32(-0.5), f32(8.0), 15, 1), (f32(-np.inf), f32(8.0), 15, 1),
        (f32(np.nan), f32(8.0), 15, 1), (f32(np.inf), f32(8.0), 15, 16), (f32(np.inf), f32(0.0), 15, 1),   # inf * 0 is NaN
        (f32(0.7), tiny, 15, 1), (f32(3.0e38), tiny, 15, 1), (f32(3.0e38), f32(3.0e38), 15, 16),        # underflow, overflow
        (f32(0.7), f32(0.0), 15, 1), (f32(0.7), f32(8.0), 0, 1), (f32(0.124), f32(8.0), 15, 1), (f32(0.125), f32(8.0), 15, 2),
    ]


def test_the_quantisation_at_its_edges():
    for cell, gain, maxp, m in edge_values():
        assert int(PC.multiplier(np.array([[cell]], dtype=f32), gain, maxp)[0, 0]) == m, (cell, gain, maxp)
    assert ROUNDS_UP[0] * ROUNDS_UP[1] == f32(4.0) and float(ROUNDS_UP[0]) * float(ROUNDS_UP[1]) < 4.0
    # a NaN cell is blocked before its multiplier is asked for; a negative cell is free and costs what a zero costs
    cells = np.array([[0.0, np.nan, 0.0], [0.0, -2.0, 0.0], [0.0, 0.5, 0.0]], dtype=f32)
    D = PC.field_dijkstra(cells, (2, 1), 0.75, 8.0, 15)
    assert D[0, 1] == PR.BLOCKED and D[1, 1] == 5 and D[2, 1] == 5 * 5 + 5 and D[1, 0] == 10 and D[2, 0] == 12


def test_numpys_plan_multiplier_is_the_checker():
    for cell, gain, maxp, m in edge_values():
        got = batch.plan_multiplier(np.array([[cell]], dtype=f32), gain, maxp)
        assert got.dtype == np.int32 and got.shape == (1, 1) and int(got[0, 0]) == m, (cell, gain, maxp)
    rng = np.random.default_rng(3)
    cells = (rng.random((40, 50)) * 1.2 - 0.1).astype(f32)
    for gain, maxp in ((GAIN, 15), (3.0, 2), (100.0, 15), (0.0, 9)):
        assert (batch.plan_multiplier(cells, gain, maxp) == PC.multiplier(cells, gain, maxp)).all()
    for bad in (-1, 16):
        with pytest.raises(ValueError):
            batch.plan_multiplier(cells, 1.0, bad)


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan_cost") / "plan_penalty_check")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", build.CSRC, os.path.join(ROOT, "tools", "plan_penalty_check.cpp"), "-o", out], check=True)
    return out


def test_the_devices_quantisation_is_the_checker(check_program):
    cases = [(cell, gain, maxp) for cell, gain, maxp, _ in edge_values()]
    rng = np.random.default_rng(19)
    for _ in range(400):
        gain = f32(rng.choice([0.0, 1.0, 3.0, GAIN, 30.0, 1.0e-3, 255.0])) * f32(rng.choice([1.0, rng.random() + 0.5]))
        cell = f32(rng.choice([rng.random() * 1.5 - 0.2, int(rng.integers(0, 9)) * 0.09375]))
        cases.append((cell, gain, int(rng.integers(0, 16))))
    lines = ["%s %s %d" % (float(c).hex(), float(g).hex(), m) for c, g, m in cases]
    out = subprocess.run([check_program], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(cases) + 1
    for (c, g, m), line in zip(cases, out):
        assert int(line) == int(PC.multiplier(np.array([c], dtype=f32), g, m)[0]), (c, g, m, line)


# ---- the spec's two cases ----------------------------------------------------------------------------------------------------------
def _route(cells, start, goal, gain, maxp, wrong=None):
    pose = (PR.ORIGIN[0] + (start[0] + 0.5) * PR.RES, PR.ORIGIN[1] + (start[1] + 0.5) * PR.RES)
    r = PC.plan(cells, PR.ORIGIN, PR.RES, pose, goal, PR.LETHAL, PR.MAX_POSES, gain, maxp, wrong)
    return r, (None if r["path"] is None else PC.route_cells(r["path"], PR.ORIGIN, PR.RES))


def test_the_clearance_case():
    cells, start, goal = PC.clearance_case()
    r0, route0 = _route(cells, start, goal, 0.0, 15)
    assert r0["status"] == PR.OK and r0["dist"] == 44
    assert route0 == [(0, 3), (1, 3), (2, 3), (3, 4), (4, 4), (5, 4), (6, 4), (7, 4), (8, 3)]
    r1, route1 = _route(cells, start, goal, 8.0, 15)
    assert r1["status"] == PR.OK and r1["dist"] == 48
    assert route1 == [(0, 3), (1, 3), (2, 4), (3, 5), (4, 5), (5, 5), (6, 5), (7, 4), (8, 3)]
    ring = lambda route: sum(cells[y, x] == 0.5 for x, y in route)
    assert ring(route0) == 3 and ring(route1) == 0


def test_the_saturating_row():
    cells = np.full((1, 900), 0.5, dtype=f32)
    assert (PC.multiplier(cells, 30.0, 15) == 16).all()
    D = PC.field_dijkstra(cells, (0, 0), PR.LETHAL, 30.0, 15)
    assert D[0, 819] == 65520 and D[0, 820] == PR.FAR and D[0, 899] == PR.FAR and D[0, 1] == 80
    assert (D == PC.field_jacobi(cells, (0, 0), PR.LETHAL, 30.0, 15)[0]).all()
    at = lambda x: (PR.ORIGIN[0] + (x + 0.5) * PR.RES, PR.ORIGIN[1] + 0.5 * PR.RES)
    far = PC.plan(cells, PR.ORIGIN, PR.RES, at(820), (0, 0), PR.LETHAL, PR.MAX_POSES, 30.0, 15, field=D)
    near = PC.plan(cells, PR.ORIGIN, PR.RES, at(819), (0, 0), PR.LETHAL, PR.MAX_POSES, 30.0, 15, field=D)
    assert far["status"] == PR.UNREACHABLE and far["dist"] == PR.FAR and far["path"] is None
    assert near["status"] == PR.OK and near["poses"] == 820 and near["dist"] == 65520


# ---- the wrong versions -------------------------------------------------------------------------------------------------------------
def listed_cases():
    """(name, cells, start, goal, gain, max_penalty): what every wrong version is held against"""
    out = []
    cells, start, goal = PC.clearance_case()
    out.append(("clearance", cells, start, goal, 8.0, 15))
    out.append(("clearance_capped", cells, start, goal, 8.0, 2))
    out.append(("saturating_row", np.full((1, 900), 0.5, dtype=f32), (830, 0), (0, 0), 30.0, 15))
    rounds_up = np.full((1, 7), ROUNDS_UP[0], dtype=f32)
    out.append(("rounds_up", rounds_up, (0, 0), (6, 0), ROUNDS_UP[1], 15))
    halves = np.zeros((3, 7), dtype=f32)
    halves[1, 1:6] = 0.4375   # t = 3.5: truncation and rounding part
    out.append(("halves", halves, (0, 1), (6, 1), 8.0, 15))
    ties = np.zeros((5, 5), dtype=f32)
    ties[2, 2] = 0.5
    out.append(("ties", ties, (0, 0), (4, 4), 8.0, 15))
    for (nx, ny), kind in itertools.product(((7, 5), (13, 9)), ("random", "wall_with_gap", "diagonal_pair")):
        c, s, g = PR.case(kind, nx, ny, seed=nx + ny)
        out.append(("%s_%dx%d" % (kind, nx, ny), PC.graded(c, seed=nx), s, g, GAIN, 15))
    return out


@pytest.mark.parametrize("wrong", PC.WRONG)
def test_every_wrong_version_differs_on_a_listed_case(wrong):
    differs = []
    for name, cells, start, goal, gain, maxp in listed_cases():
        if _outcome(_route(cells, start, goal, gain, maxp, wrong)[0]) != _outcome(_route(cells, start, goal, gain, maxp)[0]):
            differs.append(name)
    assert differs, wrong


def test_there_are_at_least_eight_wrong_versions_and_a_right_one_is_itself():
    assert len(PC.WRONG) >= 8 and len(set(PC.WRONG)) == len(PC.WRONG)
    for name, cells, start, goal, gain, maxp in listed_cases():
        assert _outcome(_route(cells, start, goal, gain, maxp)[0]) == _outcome(_route(cells.copy(), start, goal, gain, maxp)[0]), name

"""Paths planned on the device (ccv_mppi_batch_resident_plan_enqueue), restated in Python.

The spec, integers only but for one pose-to-cell step and one cell-to-pose step.  A map has nx x ny float32 cells:

    blocked(c) = not (cell(c) <= lethal)      an fp32 compare: a NaN cell is blocked, a cell equal to lethal is free; everything
                                              outside the map is blocked
    moves      (x, y) -> (x + dx, y + dy), dx, dy in {-1, 0, 1} not both zero, weight 5 straight and 7 diagonal; allowed iff the
               target is not blocked and, for a diagonal, (x + dx, y) and (x, y + dy) are not blocked either
    field      D uint16: 65535 on blocked cells, 0 on the goal, else min(65533, least total weight of an allowed path to the goal)
    start      fx = (x - origin_x) * inv, fy likewise, inv = RN(1 / resolution); in = 0 <= fx < nx and 0 <= fy < ny; s = (int(fx), int(fy))
    descent    from s until D == 0: the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with D(n) + w == D(c)
    pose i     origin + (cell i + 0.5) * resolution, one multiplication and one addition

`blocked` is the first line; `field_dijkstra`, `field_jacobi` (which also counts its sweeps, J, the last one that changes nothing
included) and `field_bellman_ford` three ways to the one field; `pose_cell` the start, `descend` the descent, `plan` the whole
with the status of include/ccv_mppi_plan.h.  `wrong` names a deliberately wrong version, for tests/test_plan_reference.py.  The
map makers and case lists at the end are what that test and tests/test_gpu_batch_plan.py run.
"""
import heapq

import numpy as np

BLOCKED, FAR = 65535, 65533
MAX_FIELD, MAX_POSES = 81920, 16384   # CCV_MPPI_PLAN_MAX_FIELD, _MAX_POSES
OK, TRUNCATED, NO_START, START_BLOCKED, GOAL_BLOCKED, UNREACHABLE, NOT_CONVERGED = 1, 2, 3, 4, 5, 6, 7
WRONG = ("four_connected", "weights_1_1", "weights_5_8", "corner_cutting", "tie_reversed", "ge_blocked", "nan_free", "clip_65535",
         "centre_no_half", "goal_first", "start_round")   # values of `wrong`
# (dx, dy) in the descent's order: E, N, W, S, NE, NW, SW, SE
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))


def weights(wrong=None):
    """(straight, diagonal)"""
    return {"weights_1_1": (1, 1), "weights_5_8": (5, 8)}.get(wrong, (5, 7))


def moves(wrong=None):
    return MOVES[:4] if wrong == "four_connected" else MOVES


def blocked(cells, lethal, wrong=None):
    """bool [ny][nx]"""
    cells, lethal = np.asarray(cells, dtype=np.float32), np.float32(lethal)
    with np.errstate(invalid="ignore"):
        if wrong == "ge_blocked":
            return cells >= lethal
        if wrong == "nan_free":
            return cells > lethal
        return ~(cells <= lethal)


def _padded(blk):
    """the blocked map with a border of blocked cells, flat, and its pitch"""
    ny, nx = blk.shape
    pad = np.ones((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = blk
    return pad.ravel().tolist(), nx + 2


def _far(wrong):
    return BLOCKED if wrong == "clip_65535" else FAR


def _edges(P, wrong):
    """(offset, weight, side offsets) of every move on the padded map"""
    ws, wd = weights(wrong)
    out = []
    for dx, dy in moves(wrong):
        diag = dx != 0 and dy != 0
        out.append((dy * P + dx, wd if diag else ws, (dx, dy * P) if diag and wrong != "corner_cutting" else ()))
    return out


def _unpad(D, ny, nx):
    return np.array(D, dtype=np.uint16).reshape(ny + 2, nx + 2)[1:-1, 1:-1].copy()


def field_dijkstra(cells, goal, lethal, wrong=None):
    """uint16 [ny][nx], by Dijkstra from the goal (the move rule is symmetric) with the clip"""
    blk = blocked(cells, lethal, wrong)
    ny, nx = blk.shape
    B, P = _padded(blk)
    far, edges = _far(wrong), _edges(P, wrong)
    D = [BLOCKED if b else far for b in B]
    g = (goal[1] + 1) * P + goal[0] + 1
    if not B[g]:
        D[g] = 0
        heap = [(0, g)]
        while heap:
            d, c = heapq.heappop(heap)
            if d > D[c]:
                continue
            for off, w, sides in edges:
                n = c + off
                if B[n] or any(B[c + s] for s in sides):
                    continue
                nd = d + w
                if nd < D[n] and nd < far:
                    D[n] = nd
                    heapq.heappush(heap, (nd, n))
    return _unpad(D, ny, nx)


def field_jacobi(cells, goal, lethal, wrong=None, max_sweeps=None):
    """(uint16 [ny][nx], J): sweeps of D'(c) = min(D(c), min(far, D(n) + w)) over all cells at once until one changes nothing; J
    counts that one too.  Stops after max_sweeps where that is given (J = max_sweeps + 1 then says: not converged)."""
    blk = blocked(cells, lethal, wrong)
    ny, nx = blk.shape
    far = _far(wrong)
    ws, wd = weights(wrong)
    pad = np.ones((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = blk
    D = np.where(pad, BLOCKED, far).astype(np.int64)
    if not blk[goal[1], goal[0]]:
        D[goal[1] + 1, goal[0] + 1] = 0
    free = ~pad[1:-1, 1:-1]
    sl = lambda dx, dy: (slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
    J = 0
    while max_sweeps is None or J < max_sweeps:
        J += 1
        new = D[1:-1, 1:-1].copy()
        for dx, dy in moves(wrong):
            diag = dx != 0 and dy != 0
            ok = free & ~pad[sl(dx, dy)]
            if diag and wrong != "corner_cutting":
                ok &= ~pad[sl(dx, 0)] & ~pad[sl(0, dy)]
            cand = np.minimum(D[sl(dx, dy)] + (wd if diag else ws), far)
            new = np.where(ok, np.minimum(new, cand), new)
        if (new == D[1:-1, 1:-1]).all():
            return new.astype(np.uint16), J
        D[1:-1, 1:-1] = new
    return D[1:-1, 1:-1].astype(np.uint16), J + 1


def field_bellman_ford(cells, goal, lethal, wrong=None):
    """uint16 [ny][nx]: every edge relaxed in a fixed order, cell by cell, until a pass changes nothing (small maps only)"""
    blk = blocked(cells, lethal, wrong)
    ny, nx = blk.shape
    B, P = _padded(blk)
    far, edges = _far(wrong), _edges(P, wrong)
    D = [BLOCKED if b else far for b in B]
    g = (goal[1] + 1) * P + goal[0] + 1
    if not B[g]:
        D[g] = 0
    changed = True
    while changed:
        changed = False
        for c in range(len(B)):
            if B[c]:
                continue
            for off, w, sides in edges:
                n = c + off
                if B[n] or any(B[c + s] for s in sides):
                    continue
                nd = min(far, D[n] + w)
                if nd < D[c]:
                    D[c], changed = nd, True
    return _unpad(D, ny, nx)


def pose_cell(x, y, origin, resolution, nx, ny, wrong=None):
    """the cell (sx, sy) the pose lies in, or None (outside the map, or not a number)"""
    inv = 1.0 / float(resolution)
    with np.errstate(invalid="ignore"):
        fx, fy = (np.float64(x) - np.float64(origin[0])) * inv, (np.float64(y) - np.float64(origin[1])) * inv
    if not (fx >= 0.0 and fx < nx and fy >= 0.0 and fy < ny):
        return None
    if wrong == "start_round":
        return min(int(np.floor(fx + 0.5)), nx - 1), min(int(np.floor(fy + 0.5)), ny - 1)
    return int(fx), int(fy)


def descend(D, start, wrong=None):
    """the cells [(x, y), ...] from `start` to the goal; D(start) must be below FAR"""
    ny, nx = D.shape
    ws, wd = weights(wrong)
    at = lambda x, y: int(D[y, x]) if 0 <= x < nx and 0 <= y < ny else BLOCKED
    order = moves(wrong)[::-1] if wrong == "tie_reversed" else moves(wrong)
    c, out = (int(start[0]), int(start[1])), []
    while True:
        out.append(c)
        d = at(*c)
        if d == 0:
            return out
        for dx, dy in order:
            diag = dx != 0 and dy != 0
            if diag and wrong != "corner_cutting" and (at(c[0] + dx, c[1]) == BLOCKED or at(c[0], c[1] + dy) == BLOCKED):
                continue
            n = at(c[0] + dx, c[1] + dy)
            if n != BLOCKED and n + (wd if diag else ws) == d:
                c = (c[0] + dx, c[1] + dy)
                break
        else:
            raise AssertionError("the field is not at its fixpoint at %r" % (c,))


def cell_poses(cells_xy, origin, resolution, wrong=None):
    """(x, y) float64 of the cells' centres: one multiplication, one addition"""
    c = np.asarray(cells_xy, dtype=np.float64).reshape(-1, 2)
    half = 0.0 if wrong == "centre_no_half" else 0.5
    return np.float64(origin[0]) + (c[:, 0] + half) * np.float64(resolution), np.float64(origin[1]) + (c[:, 1] + half) * np.float64(resolution)


def plan(cells, origin, resolution, pose, goal, lethal, capacity, wrong=None, converged=True, field=None):
    """One instance's plan as ccv_mppi_batch_resident_read_plan and _read_path report it: a dict of status, poses (L, or 0),
    start ((sx, sy), or (-1, -1)), dist (D(start), or -1), path ((x, y) of the min(L, capacity) poses that replace the path, or
    None: the path stays) and field (or None where none is built).  converged=False: the sweeps ran out.  field: D where the
    caller has it already."""
    cells = np.asarray(cells, dtype=np.float32)
    ny, nx = cells.shape
    out = dict(status=0, poses=0, start=(-1, -1), dist=-1, path=None, field=None)
    s = pose_cell(pose[0], pose[1], origin, resolution, nx, ny, wrong)
    blk = blocked(cells, lethal, wrong)
    if s is None:
        return dict(out, status=NO_START)
    out["start"] = s
    if blk[s[1], s[0]]:
        return dict(out, status=START_BLOCKED)
    if blk[goal[1], goal[0]]:
        return dict(out, status=GOAL_BLOCKED)
    if not converged:
        return dict(out, status=NOT_CONVERGED)
    D = field_dijkstra(cells, goal, lethal, wrong) if field is None else field
    out["field"], out["dist"] = D, int(D[s[1], s[0]])
    if out["dist"] >= FAR:
        return dict(out, status=UNREACHABLE)
    route = descend(D, s, wrong)
    if wrong == "goal_first":
        route = route[::-1]
    x, y = cell_poses(route[:capacity], origin, resolution, wrong)
    return dict(out, status=TRUNCATED if len(route) > capacity else OK, poses=len(route), path=(x, y))


# ---- maps -----------------------------------------------------------------------------------------------------------------------
LETHAL = np.float32(0.75)


def empty(nx, ny):
    return np.zeros((ny, nx), dtype=np.float32)


def random_map(nx, ny, seed=0, density=0.2, lethal=LETHAL):
    """`density` of the cells above lethal, and among the rest some NaN, some equal to lethal and some one ulp above it"""
    rng = np.random.default_rng(1000 + seed)
    cells = (rng.random((ny, nx)) * lethal * 0.9).astype(np.float32)
    kind = rng.random((ny, nx))
    cells[kind < density] = np.float32(1.0)
    cells[(kind >= density) & (kind < density + 0.03)] = np.nan
    cells[(kind >= density + 0.03) & (kind < density + 0.08)] = lethal
    cells[(kind >= density + 0.08) & (kind < density + 0.11)] = np.nextafter(np.float32(lethal), np.float32(np.inf))
    return cells


def wall_with_gap(nx, ny):
    """a wall across the map at x = nx // 2 with one free cell"""
    cells = empty(nx, ny)
    cells[:, nx // 2] = 1.0
    cells[(2 * ny) // 3, nx // 2] = 0.0
    return cells


def diagonal_pair(nx, ny):
    """two blocked cells that touch at a corner in the middle of the map: the only way between them would cut it"""
    cells = empty(nx, ny)
    x, y = max(nx // 2 - 1, 0), max(ny // 2 - 1, 0)
    cells[y, min(x + 1, nx - 1)] = 1.0
    cells[min(y + 1, ny - 1), x] = 1.0
    return cells


def serpentine(nx, ny):
    """every second row a wall with a gap at alternating ends: one corridor through all free rows"""
    cells = empty(nx, ny)
    for k, y in enumerate(range(1, ny, 2)):
        cells[y, :] = 1.0
        cells[y, nx - 1 if k % 2 == 0 else 0] = 0.0
    return cells


def enclosed(nx, ny):
    """the cells round (nx - 1, ny - 1) blocked: that corner is free and reached from nowhere"""
    cells = empty(nx, ny)
    cells[max(ny - 2, 0):, max(nx - 2, 0):] = 1.0
    cells[ny - 1, nx - 1] = 0.0
    return cells


MAKERS = {"empty": empty, "random": random_map, "wall_with_gap": wall_with_gap, "diagonal_pair": diagonal_pair, "serpentine": serpentine,
          "enclosed": enclosed}
ORIGIN, RES = (-3.0, 1.5), 0.25   # (a resolution of 2^-2 and origins that are multiples of it: a pose can sit exactly on a cell edge)


def free_cell(cells, lethal, prefer):
    """the free cell nearest to `prefer` in the row-major scan from it (wrapping), or None"""
    blk = blocked(cells, lethal)
    ny, nx = blk.shape
    k0 = prefer[1] * nx + prefer[0]
    for k in list(range(k0, nx * ny)) + list(range(k0)):
        if not blk[k // nx, k % nx]:
            return k % nx, k // nx
    return None


def case(kind, nx, ny, seed=0, finite=False):
    """(cells, start cell, goal cell) of a listed map: the start near cell (0, 0), the goal near the far corner; both free
    (the enclosed map: its goal is the enclosed corner; the random map: the first and the last cell, row by row, that the free
    cell nearest the map's centre reaches, so that neither lies in a pocket).  finite: no NaN cell."""
    cells = MAKERS[kind](nx, ny, seed) if kind == "random" else MAKERS[kind](nx, ny)
    if free_cell(cells, LETHAL, (0, 0)) is None:   # (a map too small for its pattern: one free cell)
        cells[0, 0] = 0.0
    if finite:   # (ccv_mppi_batch_set_grids takes no NaN: the same cells blocked, by a value one ulp above lethal)
        cells[np.isnan(cells)] = np.nextafter(LETHAL, np.float32(np.inf))
    if kind == "random":
        reached = np.argwhere(field_dijkstra(cells, free_cell(cells, LETHAL, (nx // 2, ny // 2)), LETHAL) < FAR)
        return cells, tuple(int(v) for v in reached[0][::-1]), tuple(int(v) for v in reached[-1][::-1])
    start = free_cell(cells, LETHAL, (0, 0))
    goal = (nx - 1, ny - 1) if kind == "enclosed" else free_cell(cells[::-1, ::-1], LETHAL, (0, 0))
    if kind != "enclosed":
        goal = (nx - 1 - goal[0], ny - 1 - goal[1])
    return cells, start, goal


# (nx, ny) of the reference's own test: every wrong version must differ on one of these with one of KINDS
SMALL_SHAPES = ((1, 1), (2, 2), (3, 3), (7, 5), (8, 8), (13, 9))
KINDS = tuple(MAKERS)

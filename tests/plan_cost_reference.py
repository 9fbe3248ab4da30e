"""Paths planned on the device with traversal weights (ccv_mppi_batch_resident_set_plan_penalty), restated
in Python on top of tests/plan_reference.py, whose spec stands in full: blocked, the eight moves, no corner cutting, the uint16
field with 65535 / 65533, the start cell, the status order, the pose formula.  Two values, gain and max_penalty, add:

    t = float32(cell(c)) * float32(gain)       one fp32 multiplication
    q(c) = 0 if not t > 0 else (max_penalty if t >= max_penalty else int(t))      truncation; a NaN t gives 0
    m(c) = 1 + q(c)
    step(c -> n) = w * m(c)                    w = 5 straight, 7 diagonal: the cell that is LEFT is charged
    field      the one fixpoint of D(c) = min(D(c), min(65533, D(n) + step(c -> n))), D(goal) = 0
    descent    the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with D(n) + step(c -> n) == D(c)

The move rule is not symmetric: D(c) is the least charge from c TO the goal, so `field_dijkstra`, which runs from the goal,
relaxes the predecessors of the cell it pops, each with the predecessor's own multiplier.  `multiplier` is the first three lines;
`field_dijkstra`, `field_jacobi` (with its count J, the last sweep that changes nothing included) and `field_bellman_ford` three
ways to the one field; `descend` the descent; `plan` the whole, returning plan_reference.plan's dict.  `wrong` names a
deliberately wrong version, for tests/test_plan_cost_reference.py; a wrong version is wrong in the field and in the descent alike,
so that its descent still finds its way down its own field.
"""
import heapq

import numpy as np

import plan_reference as PR

BLOCKED, FAR = PR.BLOCKED, PR.FAR
MAX_PENALTY = 15   # CCV_MPPI_PLAN_MAX_PENALTY
WRONG = ("charge_entered", "straight_only", "round", "no_clamp", "m_is_q", "clip_first", "tie_reversed", "symmetric", "fp64_product")


def multiplier(cells, gain, max_penalty, wrong=None):
    """int64, the shape of `cells`: m = 1 + q"""
    cells, maxp = np.asarray(cells, dtype=np.float32), int(max_penalty)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if wrong == "fp64_product":   # the product in doubles: differs where the fp32 product rounds up to an integer
            t = cells.astype(np.float64) * float(np.float32(gain))
        else:
            t = cells * np.float32(gain)
        positive = t > 0
    t = np.where(positive, t, 0).astype(np.float64)
    if wrong != "no_clamp":
        t = np.minimum(t, float(maxp))
    t = np.minimum(t, 1.0e6)   # (an unclamped product stays an integer that adds without overflow)
    q = (np.floor(t + 0.5) if wrong == "round" else np.trunc(t)).astype(np.int64)
    return q if wrong == "m_is_q" else 1 + q


def _charge(w, diag, mc, mn, wrong):
    """what the move c -> n of weight w costs: mc the multiplier of the cell that is left, mn of the cell that is entered"""
    if wrong == "charge_entered":
        return w * mn
    if wrong == "straight_only" and diag:
        return w
    if wrong == "symmetric":
        return (w * (mc + mn)) // 2
    return w * mc


def _candidate(dn, w, diag, mc, mn, wrong):
    """what D(c) may fall to through the neighbour n: min(FAR, D(n) + step)"""
    if wrong == "clip_first":   # the unweighted step clipped, the rest of the charge added afterwards: the uint16 wraps
        return (min(FAR, dn + w) + _charge(w, diag, mc, mn, wrong) - w) & 0xFFFF
    return min(FAR, dn + _charge(w, diag, mc, mn, wrong))


def _setup(cells, goal, lethal, gain, max_penalty, wrong):
    blk = PR.blocked(cells, lethal)
    ny, nx = blk.shape
    B, P = PR._padded(blk)
    M = np.ones((ny + 2, nx + 2), dtype=np.int64)
    M[1:-1, 1:-1] = multiplier(cells, gain, max_penalty, wrong)
    D = [BLOCKED if b else FAR for b in B]
    g = (goal[1] + 1) * P + goal[0] + 1
    if not B[g]:
        D[g] = 0
    return ny, nx, B, P, M.ravel().tolist(), D, g


def _u16(D, ny, nx):
    """the field as the device would store it: a wrong version's values above 65535 wrap"""
    return PR._unpad([int(d) & 0xFFFF for d in D], ny, nx)


def field_dijkstra(cells, goal, lethal, gain, max_penalty, wrong=None):
    """uint16 [ny][nx], by Dijkstra from the goal over predecessors: popping n, every c with an allowed move c -> n is relaxed
    with c's own multiplier (the candidate never lies below D(n), so the order of the pops is the order of the values)"""
    ny, nx, B, P, M, D, g = _setup(cells, goal, lethal, gain, max_penalty, wrong)
    edges = PR._edges(P, None)
    if not B[g]:
        heap = [(0, g)]
        while heap:
            d, n = heapq.heappop(heap)
            if d > D[n]:
                continue
            for off, w, sides in edges:
                c = n - off   # the move c -> n has offset off; its side cells are c + s
                if B[c] or any(B[c + s] for s in sides):
                    continue
                nd = _candidate(d, w, bool(sides), M[c], M[n], wrong)
                if nd < D[c]:
                    D[c] = nd
                    heapq.heappush(heap, (nd, c))
    return _u16(D, ny, nx)


def field_bellman_ford(cells, goal, lethal, gain, max_penalty, wrong=None):
    """uint16 [ny][nx]: every move out of every cell relaxed in a fixed order until a pass changes nothing (small maps only)"""
    ny, nx, B, P, M, D, g = _setup(cells, goal, lethal, gain, max_penalty, wrong)
    edges = PR._edges(P, None)
    changed = True
    while changed:
        changed = False
        for c in range(len(B)):
            if B[c] or c == g:
                continue
            for off, w, sides in edges:
                n = c + off
                if B[n] or any(B[c + s] for s in sides):
                    continue
                nd = _candidate(D[n], w, bool(sides), M[c], M[n], wrong)
                if nd < D[c]:
                    D[c], changed = nd, True
    return _u16(D, ny, nx)


def field_jacobi(cells, goal, lethal, gain, max_penalty, wrong=None, max_sweeps=None):
    """(uint16 [ny][nx], J): sweeps of D'(c) = min(D(c), min(FAR, D(n) + step(c -> n))) over all cells at once until one changes
    nothing; J counts that one too.  Stops after max_sweeps where that is given (J = max_sweeps + 1 then says: not converged).
    The right version only."""
    assert wrong is None
    blk = PR.blocked(cells, lethal)
    ny, nx = blk.shape
    pad = np.ones((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = blk
    D = np.where(pad, BLOCKED, FAR).astype(np.int64)
    if not blk[goal[1], goal[0]]:
        D[goal[1] + 1, goal[0] + 1] = 0
    M = multiplier(cells, gain, max_penalty)
    free = ~blk
    free[goal[1], goal[0]] = False   # (the goal stays 0)
    sl = lambda dx, dy: (slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
    J = 0
    while max_sweeps is None or J < max_sweeps:
        J += 1
        new = D[1:-1, 1:-1].copy()
        for dx, dy in PR.MOVES:
            diag = dx != 0 and dy != 0
            ok = free & ~pad[sl(dx, dy)]
            if diag:
                ok &= ~pad[sl(dx, 0)] & ~pad[sl(0, dy)]
            cand = np.minimum(D[sl(dx, dy)] + (7 if diag else 5) * M, FAR)
            new = np.where(ok, np.minimum(new, cand), new)
        if (new == D[1:-1, 1:-1]).all():
            return new.astype(np.uint16), J
        D[1:-1, 1:-1] = new
    return D[1:-1, 1:-1].astype(np.uint16), J + 1


def descend(D, start, M, wrong=None):
    """the cells [(x, y), ...] from `start` down the field D to the goal, M the multipliers [ny][nx]; D(start) must be below FAR.
    (A wrong version whose steps may cost nothing stops after MAX_POSES cells.)"""
    ny, nx = D.shape
    at = lambda x, y: int(D[y, x]) if 0 <= x < nx and 0 <= y < ny else BLOCKED
    order = PR.MOVES[::-1] if wrong == "tie_reversed" else PR.MOVES
    c, out = (int(start[0]), int(start[1])), []
    while True:
        out.append(c)
        d = at(*c)
        if d == 0 or len(out) >= PR.MAX_POSES:
            return out
        for dx, dy in order:
            diag = dx != 0 and dy != 0
            if diag and (at(c[0] + dx, c[1]) == BLOCKED or at(c[0], c[1] + dy) == BLOCKED):
                continue
            n = at(c[0] + dx, c[1] + dy)
            if n == BLOCKED:
                continue
            if (_candidate(n, 7 if diag else 5, diag, int(M[c[1], c[0]]), int(M[c[1] + dy, c[0] + dx]), wrong) & 0xFFFF) == d:
                c = (c[0] + dx, c[1] + dy)
                break
        else:
            if wrong is None:
                raise AssertionError("the field is not at its fixpoint at %r" % (c,))
            return out


def plan(cells, origin, resolution, pose, goal, lethal, capacity, gain, max_penalty, wrong=None, converged=True, field=None):
    """plan_reference.plan with the multipliers of (gain, max_penalty): the same dict of status, poses, start, dist, path, field"""
    cells = np.asarray(cells, dtype=np.float32)
    ny, nx = cells.shape
    out = dict(status=0, poses=0, start=(-1, -1), dist=-1, path=None, field=None)
    s = PR.pose_cell(pose[0], pose[1], origin, resolution, nx, ny)
    blk = PR.blocked(cells, lethal)
    if s is None:
        return dict(out, status=PR.NO_START)
    out["start"] = s
    if blk[s[1], s[0]]:
        return dict(out, status=PR.START_BLOCKED)
    if blk[goal[1], goal[0]]:
        return dict(out, status=PR.GOAL_BLOCKED)
    if not converged:
        return dict(out, status=PR.NOT_CONVERGED)
    D = field_dijkstra(cells, goal, lethal, gain, max_penalty, wrong) if field is None else field
    out["field"], out["dist"] = D, int(D[s[1], s[0]])
    if out["dist"] >= FAR:
        return dict(out, status=PR.UNREACHABLE)
    route = descend(D, s, multiplier(cells, gain, max_penalty, wrong), wrong)
    x, y = PR.cell_poses(route[:capacity], origin, resolution)
    return dict(out, status=PR.TRUNCATED if len(route) > capacity else PR.OK, poses=len(route), path=(x, y))


def route_cells(path, origin, resolution):
    """the cells [(x, y), ...] of a planned path's poses (cell centres)"""
    x, y = path
    return [(int(np.floor((a - origin[0]) / resolution)), int(np.floor((b - origin[1]) / resolution))) for a, b in zip(x, y)]


# ---- maps -----------------------------------------------------------------------------------------------------------------------
def graded(cells, lethal=PR.LETHAL, seed=0):
    """a listed map of plan_reference with its free cells graded: the same cells blocked, every free cell a multiple of
    lethal / 8 below lethal (so that gain = 8 / lethal puts many products on an integer), the cells beside a blocked one higher"""
    cells = np.array(cells, dtype=np.float32)
    blk = PR.blocked(cells, lethal)
    rng = np.random.default_rng(500 + seed)
    steps = rng.integers(0, 4, size=cells.shape)
    pad = np.zeros((cells.shape[0] + 2, cells.shape[1] + 2), dtype=bool)
    pad[1:-1, 1:-1] = blk
    near = np.zeros_like(blk)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= pad[dy:dy + cells.shape[0], dx:dx + cells.shape[1]]
    steps = np.where(near, steps + 4, steps)
    keep = (cells == lethal) & ~blk   # (the cells at lethal stay there: free, with the largest product)
    out = np.where(blk | keep, cells, (steps * (np.float32(lethal) / np.float32(8))).astype(np.float32))
    return out.astype(np.float32)


def clearance_case():
    """(cells, start, goal): the 9 x 7 map with one obstacle cell and its ring of half-cost cells"""
    cells = np.zeros((7, 9), dtype=np.float32)
    cells[2:5, 3:6] = 0.5
    cells[3, 4] = 1.0
    return cells, (0, 3), (8, 3)

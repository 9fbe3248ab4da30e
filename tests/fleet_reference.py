"""The fleet term's selection (ccv_mppi_batch_resident_set_fleet), the spec literally: which other
robots of a resident batch become discs of robot y's list in one tick, in what order and with what radius.

    dx = q_j[0] - q_y[0], dy = q_j[1] - q_y[1], d2 = dx*dx + dy*dy          (fp64, no FMA)
    robot j != y is a candidate iff d2 <= range2, range2 = range*range rounded once (a NaN fails)
    the candidates in (d2, j) order; the first M_y = min(max_neighbours, MAX_OBSTACLES - n_static[y]) are taken, in that order
    row of neighbour j: (q_j[0], q_j[1], radius[y] + radius[j]);  n_total[y] = n_static[y] + taken

q: every robot's position at the start of the tick (what _resident_read returned after the previous tick), the own one too.

Two backends.  `lists` is numpy float64 (one row of differences per robot).  `lists_exact` does every operation on exact
rationals (Fraction of the same doubles) and rounds the exact result to the nearest double after every operation: what IEEE
arithmetic is defined to give, with no floating-point instruction involved.  tests/test_fleet_reference.py pins the two
against each other and holds the wrong versions that must differ.
"""
from fractions import Fraction

import numpy as np

MAX_OBSTACLES = 32


def room(n_static, max_neighbours):
    """M_y for every robot"""
    return np.maximum(np.minimum(int(max_neighbours), MAX_OBSTACLES - np.asarray(n_static, dtype=np.int64)), 0)


def lists(q, radius, n_static, max_neighbours, rng):
    """-> (n_total [B] int32, rows: B arrays [taken_y][3] in the order written).  numpy float64."""
    q = np.asarray(q, dtype=np.float64)
    radius = np.asarray(radius, dtype=np.float64)
    B = q.shape[0]
    M = room(n_static, max_neighbours)
    with np.errstate(over="ignore"):   # (a range whose square overflows: +inf, as the host's product)
        range2 = np.float64(rng) * np.float64(rng)
    j_all = np.arange(B)
    n_total, rows = np.zeros(B, dtype=np.int32), []
    for y in range(B):
        with np.errstate(over="ignore", invalid="ignore"):   # (positions that are not finite: IEEE's results, no warning)
            dx = q[:, 0] - q[y, 0]
            dy = q[:, 1] - q[y, 1]
            d2 = dx * dx + dy * dy
            cand = (d2 <= range2) & (j_all != y)
        idx = np.flatnonzero(cand)
        take = idx[np.lexsort((idx, d2[idx]))][:M[y]]
        rows.append(np.stack([q[take, 0], q[take, 1], radius[y] + radius[take]], axis=1) if len(take) else np.zeros((0, 3)))
        n_total[y] = int(n_static[y]) + len(take)
    return n_total, rows


def _rd(f):
    """the exact rational, rounded to the nearest double (ties to even: Fraction -> float is correctly rounded)"""
    return Fraction(float(f))


def lists_exact(q, radius, n_static, max_neighbours, rng):
    """the same from exact rationals, rounded after every operation.  Finite inputs only."""
    q = np.asarray(q, dtype=np.float64)
    B = q.shape[0]
    Q = [(Fraction(float(x)), Fraction(float(y))) for x, y in q]
    Rd = [Fraction(float(r)) for r in radius]
    M = room(n_static, max_neighbours)
    range2 = _rd(Fraction(float(rng)) * Fraction(float(rng)))
    n_total, rows = np.zeros(B, dtype=np.int32), []
    # every operation is done once per pair of operands (a lattice of a thousand robots has few distinct differences); a rounded
    # result is a double, and the comparisons below compare those doubles: the same order as the rationals'
    Qf = q.tolist()
    range2 = float(range2)
    diff, key = {}, {}

    def sub(a, b, k):
        if k not in diff:
            r = _rd(a - b)
            diff[k] = (r, float(r))
        return diff[k]

    for y in range(B):
        cands = []
        for j in range(B):
            if j == y:
                continue
            dx, dxf = sub(Q[j][0], Q[y][0], (Qf[j][0], Qf[y][0]))
            dy, dyf = sub(Q[j][1], Q[y][1], (Qf[j][1], Qf[y][1]))
            if (dxf, dyf) not in key:
                key[(dxf, dyf)] = float(_rd(_rd(dx * dx) + _rd(dy * dy)))
            d2 = key[(dxf, dyf)]
            if d2 <= range2:
                cands.append((d2, j))
        cands.sort()
        take = [j for _, j in cands[:M[y]]]
        rows.append(np.array([[q[j, 0], q[j, 1], float(_rd(Rd[y] + Rd[j]))] for j in take]).reshape(-1, 3))
        n_total[y] = int(n_static[y]) + len(take)
    return n_total, rows


def full_lists(static, rows):
    """robot y's whole list: its static discs [n_static_y][3], then the tick's neighbour rows"""
    return [np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3), r]) for s, r in zip(static, rows)]


def table(static, rows):
    """the lists as ccv_mppi_batch_resident_read_fleet returns them: [B][MAX_OBSTACLES][3], rows past the count zero"""
    out = np.zeros((len(rows), MAX_OBSTACLES, 3))
    for y, d in enumerate(full_lists(static, rows)):
        out[y, :len(d)] = d
    return out

"""The fleet prediction's velocity rule (ccv_mppi_batch_set_fleet_prediction), the spec literally, beside
fleet_reference.py (the selection, which prediction does not change).

    inv_dt = 1 / dt                                   (fp64, rounded once: what the step carries)
    vx = (x_after - x_before) * inv_dt,  vy alike      (one subtraction, one multiplication, no FMA)
    v = (0, 0) when the tick does not advance, when dt = 0, or when vx or vy is not finite

before / after: the robot's position at the start of the tick and after its advance -- what _resident_read returns before and
after the tick.  The velocity a tick forms is charged by the NEXT tick's rollout, in the velocity row of every disc row that
holds the robot.

Two backends: `velocity` is numpy float64; `velocity_exact` does both operations on exact rationals and rounds after each
(overflow to infinity as IEEE).  `lists` is fleet_reference.lists with the indices of the taken robots, so that a velocity row
can be put beside every disc row.
"""
from fractions import Fraction

import numpy as np

import fleet_reference as FR

DBL_MAX = Fraction(np.finfo(np.float64).max)


def velocity(before, after, dt, advance):
    """before, after [B][2] -> v [B][2], numpy float64"""
    before, after = np.asarray(before, dtype=np.float64), np.asarray(after, dtype=np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv_dt = np.float64(1.0) / np.float64(dt)
        v = (after - before) * inv_dt
    ok = bool(advance) and dt != 0.0
    good = np.isfinite(v).all(axis=1, keepdims=True) & ok
    return np.where(good, v, 0.0)


def _rd(f):
    """the exact rational rounded to the nearest double; beyond the largest double: infinity"""
    if abs(f) > DBL_MAX:
        # (round-to-nearest overflows once the magnitude reaches DBL_MAX + half an ulp; the cases below are far beyond it)
        return float("inf") if f > 0 else float("-inf")
    return float(f)


def velocity_exact(before, after, dt, advance):
    """the same from exact rationals, rounded after every operation.  Finite positions, dt >= 0."""
    before, after = np.asarray(before, dtype=np.float64), np.asarray(after, dtype=np.float64)
    out = np.zeros(before.shape)
    if not advance or dt == 0.0:
        return out
    inv_dt = _rd(Fraction(1) / Fraction(float(dt)))
    for i in range(before.shape[0]):
        v = []
        for c in range(2):
            d = _rd(Fraction(float(after[i, c])) - Fraction(float(before[i, c])))
            v.append(d * inv_dt if not np.isfinite(inv_dt) else _rd(Fraction(d) * Fraction(inv_dt)))
        if np.isfinite(v[0]) and np.isfinite(v[1]):
            out[i] = v
    return out


def lists(q, radius, n_static, max_neighbours, rng):
    """fleet_reference.lists, and per robot the indices of the taken robots in the order written"""
    q = np.asarray(q, dtype=np.float64)
    B = q.shape[0]
    M = FR.room(n_static, max_neighbours)
    with np.errstate(over="ignore"):
        range2 = np.float64(rng) * np.float64(rng)
    n_total, rows = FR.lists(q, radius, n_static, max_neighbours, rng)
    taken = []
    for y in range(B):
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy = q[:, 0] - q[y, 0], q[:, 1] - q[y, 1]
            d2 = dx * dx + dy * dy
            idx = np.flatnonzero((d2 <= range2) & (np.arange(B) != y))
        taken.append(idx[np.lexsort((idx, d2[idx]))][:M[y]])
        assert q[taken[-1]].tobytes() == rows[y][:, :2].tobytes()
    return n_total, rows, taken


def velocity_rows(static_v, taken, v):
    """robot y's velocity rows: its static discs' [n_static_y][2], then the taken neighbours' velocities"""
    return [np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2), v[t].reshape(-1, 2)]) for s, t in zip(static_v, taken)]


def table(vrows):
    """the rows as ccv_mppi_batch_read_fleet_velocities returns them: [B][MAX_OBSTACLES][2], rows past the count zero"""
    out = np.zeros((len(vrows), FR.MAX_OBSTACLES, 2))
    for y, d in enumerate(vrows):
        out[y, :len(d)] = d
    return out

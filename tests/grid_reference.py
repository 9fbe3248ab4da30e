"""The occupancy-grid term of the batch handles (ccv_mppi_batch_set_grids), restated twice.

The spec, for the states (x, y) of one sample that the path term covers, in state order, AS STORED (the doubles
ccv_mppi_batch_read_candidates returns):

    inv  = 1.0 / resolution                   rounded once
    fx   = (x - origin_x) * inv               one subtraction, one multiplication, each rounded; no FMA
    fy   = (y - origin_y) * inv
    in   = fx >= 0 and fx < nx and fy >= 0 and fy < ny       false for NaN
    v_k  = cells[int(fy) * nx + int(fx)] if in else outside  float32
    G    = ((double(v_0) + double(v_1)) + ...)               fp64, sequential, from 0.0
    cost = fma(w_grid, G, cost_rest)

Every operation is an IEEE basic operation, so the device result can be held against this bit for bit.  Two backends:
`numpy` (float64 / float32 arrays, vectorised over the samples, the one the GPU tests use) and `exact` (rationals, rounded to
a double after every operation, scalar).  tests/test_grid_reference.py pins them against each other.
"""
import math
from fractions import Fraction

import numpy as np


def n_covered(model, horizon):
    """states that reach the path term: all H for diff drive and steering, the first H - 2 for full body"""
    return horizon - 2 if model == "full_body" else horizon


class Grid:
    """one map: cells[ny][nx] float32 (x fastest), origin (ox, oy), resolution, outside"""

    def __init__(self, cells, origin, resolution, outside):
        self.cells = np.ascontiguousarray(cells, dtype=np.float32)
        assert self.cells.ndim == 2
        self.ny, self.nx = self.cells.shape
        self.ox, self.oy = float(origin[0]), float(origin[1])
        self.resolution = float(resolution)
        self.outside = np.float32(outside)
        self.inv = 1.0 / self.resolution

    def as_tuple(self):
        """the form BatchController.set_grids takes"""
        return (self.cells, (self.ox, self.oy), self.resolution, float(self.outside))


# ---- numpy backend ---------------------------------------------------------------------------------------------------------
WRONG_LOOKUPS = ("le_nx", "noge0", "floor", "convfirst")


def _wrap32(f):
    """what a wrapping conversion to a 32-bit integer leaves of the whole number f (NaN, inf: 0)"""
    with np.errstate(invalid="ignore"):
        r = np.fmod(f, 2.0 ** 32)   # (exact)
    i = np.where(np.isfinite(r), r, 0.0).astype(np.int64)
    return (i + 2 ** 31) % 2 ** 32 - 2 ** 31


def lookup(g, x, y, wrong=None):
    """(v float32, in bool, flat cell index or -1) for arrays of states.  wrong: one mistake, by name -- "le_nx" (f <= n at the
    upper edge), "noge0" (no f >= 0 test), "floor" (the cell from floor(f) converted to a 32-bit integer, the range test made on
    the integers), "convfirst" (the same with the truncating conversion: the conversion before the select).  A wrong index
    stays an index (modulo the number of cells), and a conversion beyond the integers wraps."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (x - g.ox) * g.inv
        fy = (y - g.oy) * g.inv
        inside = (fx >= 0.0) & (fx < float(g.nx)) & (fy >= 0.0) & (fy < float(g.ny))
    if wrong is not None:
        assert wrong in WRONG_LOOKUPS, wrong
        with np.errstate(invalid="ignore", over="ignore"):
            if wrong in ("floor", "convfirst"):
                whole = np.floor if wrong == "floor" else np.trunc
                ix, iy = _wrap32(whole(fx)), _wrap32(whole(fy))
                inside = (ix >= 0) & (ix < g.nx) & (iy >= 0) & (iy < g.ny)
            else:
                lo = np.ones(fx.shape, dtype=bool) if wrong == "noge0" else (fx >= 0.0) & (fy >= 0.0)
                hi = (fx <= float(g.nx)) & (fy <= float(g.ny)) if wrong == "le_nx" else (fx < float(g.nx)) & (fy < float(g.ny))
                inside = lo & hi
                ix, iy = _wrap32(np.trunc(np.where(inside, fx, 0.0))), _wrap32(np.trunc(np.where(inside, fy, 0.0)))
        idx = (iy * g.nx + ix) % g.cells.size
        v = np.where(inside, g.cells.reshape(-1)[idx], g.outside).astype(np.float32)
        return v, inside, np.where(inside, idx, -1)
    ix = np.where(inside, fx, 0.0).astype(np.int64)   # (truncation; exact for 0 <= f < 32 768)
    iy = np.where(inside, fy, 0.0).astype(np.int64)
    idx = iy * g.nx + ix
    v = np.where(inside, g.cells.reshape(-1)[idx], g.outside).astype(np.float32)
    return v, inside, np.where(inside, idx, -1)


def grid_sum(g, P, wrong=None):
    """G [K] for states P [K][n][2] (already cut to the covered states), sequential in state order"""
    P = np.asarray(P, dtype=np.float64)
    v, _, _ = lookup(g, P[..., 0], P[..., 1], wrong)
    G = np.zeros(P.shape[0], dtype=np.float64)
    for k in range(P.shape[1]):
        G = G + v[:, k].astype(np.float64)
    return G


def fma(a, b, c):
    """fma(a, b, c) of three doubles, correctly rounded (rationals; the non-finite cases by IEEE's rules)"""
    a, b, c = float(a), float(b), float(c)
    if math.isfinite(a) and math.isfinite(b) and not math.isfinite(c):
        return c   # (the exact product is finite)
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))   # (the product is inf or NaN: nothing is rounded)
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        # an exact zero sum: +0 unless both addends are -0 (round to nearest)
        prod_neg = (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0
        if a * b == 0.0 and c == 0.0:
            return -0.0 if (prod_neg and math.copysign(1.0, c) < 0) else 0.0
        return 0.0
    return _to_double(r)


def _to_double(r):
    try:
        return float(r)   # int / int true division: correctly rounded
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def cost_on(cost_off, w, G):
    """fma(w, G, cost_off) element by element"""
    cost_off, G = np.asarray(cost_off, dtype=np.float64), np.asarray(G, dtype=np.float64)
    return np.array([fma(w, G[i], cost_off[i]) for i in range(len(G))], dtype=np.float64)


# ---- exact backend ---------------------------------------------------------------------------------------------------------
def _rn(r):
    return _to_double(r)


def lookup_exact(g, x, y):
    """(v float32, in, flat index or -1) for one state; every operation in rationals, rounded to a double afterwards"""
    x, y = float(x), float(y)
    if not (math.isfinite(x) and math.isfinite(y)):
        # x - origin is x itself (inf, or NaN) and so is its product with inv > 0: NaN fails every compare, +inf fails
        # `< nx`, -inf fails `>= 0` -- unless the OTHER coordinate alone decides, which `and` does not allow
        return g.outside, False, -1
    inv = _rn(Fraction(1) / Fraction(g.resolution))
    fx = _rn(Fraction(_rn(Fraction(x) - Fraction(g.ox))) * Fraction(inv))
    fy = _rn(Fraction(_rn(Fraction(y) - Fraction(g.oy))) * Fraction(inv))
    if not (math.isfinite(fx) and math.isfinite(fy)):
        return g.outside, False, -1
    inside = Fraction(fx) >= 0 and Fraction(fx) < g.nx and Fraction(fy) >= 0 and Fraction(fy) < g.ny
    if not inside:
        return g.outside, False, -1
    ix, iy = math.trunc(Fraction(fx)), math.trunc(Fraction(fy))
    idx = iy * g.nx + ix
    return g.cells.reshape(-1)[idx], True, idx


def grid_sum_exact(g, P):
    """G of ONE sample's states P [n][2]"""
    G = 0.0
    for k in range(len(P)):
        v, _, _ = lookup_exact(g, P[k][0], P[k][1])
        G = _rn(Fraction(G) + Fraction(float(v)))
    return G


# ---- the maps of the GPU tests ---------------------------------------------------------------------------------------------
def map_ahead(pose, v_ref, dt, horizon, salt=0, ahead=0.5, backwards=False):
    """A map placed from a pose (x, y, yaw): it covers the start of the fan and ends about ahead * v_ref * dt * (H - 1) in front
    of it -- behind it with `backwards`, for a fan whose warm start drives in reverse.  Axis-aligned: the bounding box of the
    segment from the pose to that point, padded by a tenth of its length; cells of a 24th of the length; nx != ny, neither a
    power of two (a column or row more where needed); every cell a distinct small integer, `outside` a value no cell has.
    (ahead = 0.5: with 0.6 the full-body fans of the GPU tests left under 5 % of their states out of bounds on the oracle's
    rollouts, tests/test_grid_reference.py; the map was moved, the condition stayed.)"""
    x, y, yaw = float(pose[0]), float(pose[1]), float(pose[2])
    L = ahead * v_ref * dt * (horizon - 1)
    sgn = -1.0 if backwards else 1.0
    ex, ey = x + sgn * L * math.cos(yaw), y + sgn * L * math.sin(yaw)
    pad = 0.1 * L
    lo_x, hi_x = min(x, ex) - pad, max(x, ex) + pad
    lo_y, hi_y = min(y, ey) - pad, max(y, ey) + pad
    res = L / (24.0 + salt)
    nx, ny = int(math.ceil((hi_x - lo_x) / res)), int(math.ceil((hi_y - lo_y) / res))

    def pow2(n):
        return n & (n - 1) == 0

    while pow2(nx):
        nx += 1
    while pow2(ny) or ny == nx:
        ny += 1
    cells = (1.0 + np.arange(nx * ny, dtype=np.float64)).reshape(ny, nx).astype(np.float32)
    return Grid(cells, (lo_x, lo_y), res, -2.5 - salt)


def map_over(P, salt=0):
    """A map placed from the rollouts themselves: P [K][n][2], the covered states of one instance (the oracle's).  The box
    between the 10 % and the 90 % quantile of the states per axis -- so a share of the fan lies inside and a share outside
    whatever the horizon, the model and the way the warm start drives -- cells of a (36 + salt)-th of its longer side; as
    map_ahead: nx != ny, neither a power of two, every cell a distinct small integer, `outside` a value no cell has.  One map
    per instance: the horizon sweeps (tests/test_gpu_horizon_sweep_batch.py) use it where map_ahead's fixed reach misses the
    conditions on the inputs at short or odd horizons."""
    P = np.asarray(P, dtype=np.float64)
    lo_x, hi_x = (float(q) for q in np.quantile(P[..., 0], (0.1, 0.9)))
    lo_y, hi_y = (float(q) for q in np.quantile(P[..., 1], (0.1, 0.9)))
    res = max(hi_x - lo_x, hi_y - lo_y) / (36.0 + salt)
    nx, ny = max(1, int(math.ceil((hi_x - lo_x) / res))), max(1, int(math.ceil((hi_y - lo_y) / res)))

    def pow2(n):
        return n & (n - 1) == 0

    while pow2(nx):
        nx += 1
    while pow2(ny) or ny == nx:
        ny += 1
    cells = (1.0 + np.arange(nx * ny, dtype=np.float64)).reshape(ny, nx).astype(np.float32)
    return Grid(cells, (lo_x, lo_y), res, -2.5 - salt)


def coverage(g, P):
    """(share of the states in bounds, share out of bounds, distinct cells hit) over states P [K][n][2]"""
    _, inside, idx = lookup(g, P[..., 0], P[..., 1])
    return float(np.mean(inside)), float(np.mean(~inside)), int(len(np.unique(idx[inside])))

"""Reference of the batch handles' disc-obstacle term and the rounding bound of the device spec (test helper, CPU only; the
conventions of rollout_reference.py and update_reference.py).

The term (include/ccv_mppi.h, ccv_mppi_batch_set_obstacles).  For a state at the fp64 position
P = (X, Y), discs (ox_j, oy_j, r_j), j < n, and a weight w >= 0:

    power(P)   = min_j ( |P - o_j|^2 - r_j^2 )            (+inf for n = 0)
    penalty(P) = w * max(-power(P), 0)                      (0 for a NaN position)

as real-number functions of the fp64 inputs.  Arithmetic: numpy.longdouble where it has a 64-bit mantissa; every difference,
square and sum then carries a relative error of 2^-64, 2^-11 of fp64's, which REF_ULPS below charges to the bound; elsewhere
exact rationals (fractions.Fraction; `backend="exact"` forces them, and the pinning test holds the two together).

The device spec (u = 2^-53; x0 the pose the kernel holds, fl() one fp64 rounding, every fma written out):

    staging   dx = fl(ox - x0x), dy = fl(oy - x0y);  a = -2 dx, b = -2 dy (exact);  c = fl(fma(dx, dx, fl(dy dy)) - fl(r r))
              the list padded to a multiple of 4 with a = b = 0, c = +inf
    state     p = (fl(X - x0x), fl(Y - x0y))                 the pose-relative position the path term uses
              f_j = fma(a_j, p_x, fma(b_j, p_y, c_j));  m = min_j f_j;  s = fl(m + fma(p_x, p_x, fl(p_y p_y)))
              g = max(-s, 0) (NaN -> 0);  cost = fma(w, g, cost)

The bound of s, term by term, against power(P) = |p* - d*|^2 - r^2 with the unrounded p* = P - x0, d* = o - x0.  Second-order
terms are dropped and every count rounded up to make room for them.  With |d|^2 = dx^2 + dy^2, |p|^2 = p_x^2 + p_y^2:

    c     fl(dy dy): u dy^2;  the fma: u |d|^2;  fl(r r): u r^2;  the subtraction: u |c| <= u (|d|^2 + r^2);  the roundings of
          dx, dy themselves move d^2 by 2 u |d|^2                                                    <= 5 u (|d|^2 + r^2)
    f_j   the inner fma: u (|b p_y| + |c|);  the outer one: u (|a p_x| + |b p_y| + |c|);  a, b and p_x, p_y each carry one
          rounding: 2 u (|a p_x| + |b p_y|);  with |c| <= |d|^2 + r^2 and c's own error
                                                                       <= u [4 (|a p_x| + |b p_y|) + 7 (|d|^2 + r^2)]
    |p|^2 fl(p_y p_y) and the fma: 2 u |p|^2;  the roundings of p: 2 u |p|^2                         <= 4 u |p|^2
    s     the sum: u |s| <= u (|a p_x| + |b p_y| + |d|^2 + r^2 + |p|^2)
    min   |min_j f_j - min_j f*_j| <= max_j |f_j - f*_j|

    |s - power(P)| <= 8 u S,   S = max_j ( dx_j^2 + dy_j^2 + r_j^2 + |a_j p_x| + |b_j p_y| ) + |p|^2

S is a sum of magnitudes, not s: near a disc's edge the term is a difference of large numbers and the bound is absolute.  The
negation and the maximum are exact, so g carries the same bound; S_ULPS = 9 is the 8 above and one for the dropped terms.

    penalty of one state     w (S_ULPS u + REF_ULPS 2^-64) S
    sum over a sample's T states, accumulated by fma onto a running cost that starts at 0:
                             sum_t of the above + T u (sum_t penalty_t)      (every partial sum <= the total; one rounding each)

The difference of two runs (bound_difference).  A kernel with the term adds the same path, speed, ... terms, bit for bit (same
states, same controls), and T penalties, to a running sum in another order of roundings.  Each of the two costs is a sum of at
most N = 6 H + 8 non-negative terms (full body: five per step and the yaw term; the four waves' parts; the penalties), so it
differs from the real sum of its rounded terms by at most N u cost, and

    |(cost_on - cost_off) - sum_t fl-penalty_t| <= N u (cost_on + cost_off)

They are derived, not tuned.  test_obstacle_reference.py shows a numpy restatement of the spec inside them and seven wrong
versions outside.
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
HAVE_LD = np.finfo(LD).nmant >= 63
S_ULPS = 9
CHUNK = 1 << 16
REF_ULPS = 12   # longdouble: two differences, two squares, two sums, the subtraction of r^2, each 2^-64 of magnitudes <= S


def _discs(discs):
    d = np.zeros((0, 3)) if discs is None else np.asarray(discs, dtype=np.float64)
    return d.reshape(-1, 3)


# ---- the two operations the device specs of the disc terms are written in (obstacle_cases.spec, moving_obstacle_reference.spec)

def fma_rational(a, b, c):
    """fl(a b + c) with one rounding (Fraction -> float is correctly rounded); non-finite operands, and a sum beyond the
    largest double, as IEEE.  An exact zero is +0.0."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


_SPLIT = 134217729.0   # 2^27 + 1 (Veltkamp)


def fma(a, b, c):
    """fma_rational's value, faster: the product as an unevaluated sum of two doubles (Dekker), then math.fsum, which rounds
    the exact sum of its three terms once.  Factors far from 1 (the splitting could overflow or the product's low part
    underflow) and non-finite operands go to fma_rational.  tests/test_edge_probe_cpu.py holds the two together."""
    a, b, c = float(a), float(b), float(c)
    if a == 0.0 or b == 0.0:
        return c + 0.0 if math.isfinite(a) and math.isfinite(b) else fma_rational(a, b, c)
    if not (1e-100 < abs(a) < 1e100 and 1e-100 < abs(b) < 1e100 and math.isfinite(c)):
        return fma_rational(a, b, c)
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    try:
        r = math.fsum((p, ((ah * bh - p) + ah * bl + al * bh) + al * bl, c))
    except OverflowError:
        return fma_rational(a, b, c)
    return r if r != 0.0 else 0.0


def fmin(a, b):   # IEEE minNum: the number of a number and a NaN
    return b if a != a else a if b != b else min(a, b)


def nanmin(a, b):   # a wrong version's minimum: a NaN operand goes through
    return math.nan if (a != a or b != b) else min(a, b)


def power(P, discs, backend=None):
    """min_j |P - o_j|^2 - r_j^2 for fp64 positions P [..., 2]: longdouble [...] (+inf without discs, NaN for a NaN position)."""
    P = np.asarray(P, dtype=np.float64)
    d = _discs(discs)
    shape = P.shape[:-1]
    if d.shape[0] == 0:
        out = np.full(shape, np.inf, dtype=LD)
        out[np.isnan(P).any(axis=-1)] = np.nan
        return out
    if backend == "exact" or (backend is None and not HAVE_LD):
        flat = P.reshape(-1, 2)
        out = np.empty(flat.shape[0], dtype=LD)
        for i, (x, y) in enumerate(flat):
            if not (np.isfinite(x) and np.isfinite(y)):
                out[i] = np.nan
                continue
            fx, fy = Fraction(float(x)), Fraction(float(y))
            q = min((fx - Fraction(float(ox))) ** 2 + (fy - Fraction(float(oy))) ** 2 - Fraction(float(r)) ** 2 for ox, oy, r in d)
            # (to longdouble through the leading double and the remainder: both conversions are exact enough -- 2^-105)
            hi = float(q)
            out[i] = LD(hi) + LD(float(q - Fraction(hi)))
        return out.reshape(shape)
    flat = P.reshape(-1, 2)
    out = np.empty(flat.shape[0], dtype=LD)
    ox, oy, r = d[:, 0].astype(LD), d[:, 1].astype(LD), d[:, 2].astype(LD)
    for i in range(0, flat.shape[0], CHUNK):   # (states x discs in pieces: K = 82 048, H = 15, n = 32 is 39 M pairs)
        X, Y = flat[i:i + CHUNK, 0].astype(LD)[:, None], flat[i:i + CHUNK, 1].astype(LD)[:, None]
        with np.errstate(invalid="ignore"):
            q = (X - ox) * (X - ox) + (Y - oy) * (Y - oy) - r * r
            out[i:i + CHUNK] = np.min(q, axis=-1)   # (np.min propagates NaN: a NaN position gives NaN)
    return out.reshape(shape)


def penalty(P, discs, w, backend=None):
    """w * max(-power, 0) per state, longdouble [...]; 0 for a NaN position and without discs."""
    s = power(P, discs, backend)
    with np.errstate(invalid="ignore"):
        g = np.where(s < 0, -s, LD(0))
    return LD(w) * g


def scale(P, x0, discs):
    """S of the module docstring per state, fp64 [...]; 0 without discs, NaN for a NaN position."""
    P = np.asarray(P, dtype=np.float64)
    d = _discs(discs)
    px, py = P[..., 0] - x0[0], P[..., 1] - x0[1]
    p2 = px * px + py * py
    if d.shape[0] == 0:
        return np.zeros(P.shape[:-1]) + 0.0 * p2
    dx, dy, r = d[:, 0] - x0[0], d[:, 1] - x0[1], d[:, 2]
    fx, fy = px.reshape(-1), py.reshape(-1)
    out = np.empty(fx.shape[0])
    for i in range(0, fx.shape[0], CHUNK):
        per = dx * dx + dy * dy + r * r + np.abs(2.0 * dx * fx[i:i + CHUNK, None]) + np.abs(2.0 * dy * fy[i:i + CHUNK, None])
        out[i:i + CHUNK] = np.max(per, axis=-1)
    return out.reshape(px.shape) + p2


def bound_s(P, x0, discs):
    """|device s - power| per state (states with discs and a finite position)."""
    return (S_ULPS * U + REF_ULPS * 2.0 ** -64) * scale(P, x0, discs) * (1.0 + 2.0 ** -20)


def bound_penalty(P, x0, discs, w):
    """|w * device g - penalty| per state; 0 for a NaN position (the device's 0 is exact)."""
    b = float(w) * bound_s(P, x0, discs)
    return np.where(np.isnan(b), 0.0, b)


def sample_penalty(P, x0, discs, w, backend=None):
    """P [K][T][2] -> (sum_t penalty [K] as longdouble, its bound [K]) for the fma chain onto a cost that starts at 0."""
    pen = penalty(P, discs, w, backend)
    tot = pen.sum(axis=-1)
    T = pen.shape[-1]
    bnd = bound_penalty(P, x0, discs, w).sum(axis=-1) + (T + 1) * U * tot.astype(np.float64)
    return tot, bnd


def bound_difference(cost_on, cost_off, H):
    """The roundings of two differently ordered running sums (module docstring), per sample."""
    return (6 * H + 8) * U * (np.abs(cost_on) + np.abs(cost_off))

"""Extended-precision reference of the weighted update, the rounding bound of any fp64 evaluation of it, and how much a
lost or misplaced sample would move the result (test helper, CPU only).

    w_k = exp(-(c_k - shift) / lambda)     S = sum_k w_k     V[n] = sum_k w_k u_k[n]     A[n] = sum_k w_k |u_k[n]|
    u_ref = V / S

from the arrays a handle reads back: costs [K], controls [K][H-1][udim] (any trailing shape; flattened to rows n).

Arithmetic.  numpy.longdouble where it has a 64-bit mantissa (x87: nmant = 63): weights by expl, sums by numpy's pairwise
summation in longdouble -- relative error of the result a few 2^-64 * (1 + max |c/lambda|), pinned against exact rational
arithmetic in test_update_reference.py.  Where longdouble is narrower (nmant < 63) the helper does NOT drop to fp64: it
evaluates the same quantities with mpmath at 80 bits (exp) and fractions.Fraction (exact sums of exact products), which is
slow but correct; `backend="exact"` forces that path (400 bits for exp) and is what the pinning test compares against.

Rounding bound (u = 2^-53), for ANY fp64 evaluation that forms K products and adds them in any order (a tree of partial
sums per lane, wave, workgroup, chunk and rank is one such order):

    bound[n] = ((2K + 4) + 2 (X + 2 + E)) * u * A[n] / S          X = max_k |(c_k - shift) / lambda|  (* 2 with a shift)

(K-1)u for each of the two sums whatever their order, one rounding per product, one for the division; per weight X*u from
the rounded quotient -total/lambda (with a shift the rounded difference c - shift adds as much again: X counts twice)
and E ulps of the device's exp.  It is derived, not tuned.  sum_w alone: ((K + 1) + X + E) * u * S.

Weights.  |w^_k - w_k| <= (|x_k| + 2E + 2) * u * w_k for the device's normalised weights times sum_w (+2: the normalisation
and the multiplication back), with an absolute floor of 2^-1074 * (E + 1).  Subnormal handling: below 2^-1022 a double
keeps fewer bits, so the relative part of the bound is not meaningful there and the floor (E + 1 units of the smallest
subnormal) takes over; a device weight may be exactly 0 only where the reference weight, enlarged by its relative bound,
is below 2^-1074 (the smallest subnormal; anything below half of it must round to 0, between the two either is accepted),
which is what zero_count_range() brackets.

E.  The ROCm installation carries no accuracy table for the double-precision exp of the device library, so E is measured:
measured_exp_ulps() returns the largest (|w^_k - w_k| / (u w_k) - |x_k| - 2) / 2 over the normal-range weights, rounded up
to an integer >= 1.  More than E_MAX = 4 is a finding, not a tolerance.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
E_MAX = 4
LD = np.longdouble
HAVE_LD64 = np.finfo(LD).nmant >= 63
TINY = 2.0 ** -1074          # smallest subnormal double


class UpdateRef:
    """S, V, A, u_ref (longdouble arrays, or exact values rounded to longdouble) and what the bounds need."""

    def __init__(self, K, lam, shift, S, V, A, xmax):
        self.K, self.lam, self.shift = int(K), float(lam), float(shift)
        self.S, self.V, self.A = S, V, A
        self.u = V / S
        self.xmax = float(xmax) * (2.0 if shift != 0.0 else 1.0)

    # ---- bounds (fp64 arrays) ----
    def bound_u(self, E=1):
        return np.asarray(((2 * self.K + 4) + 2 * (self.xmax + 2 + E)) * U * (self.A / self.S), dtype=np.float64)

    def bound_V(self, E=1):
        """the same without the division term and S's own sum: K-1 additions, one rounding per product, the weights"""
        return np.asarray(((self.K + 1) + (self.xmax + E)) * U * self.A, dtype=np.float64)

    def bound_S(self, E=1):
        return float(((self.K + 1) + self.xmax + E) * U * self.S)

    def err_over_bound(self, u_dev, E=1):
        """max_n |u_dev[n] - u_ref[n]| / bound[n] (rows with A[n] == 0, a control dimension forced to 0, must be exact)."""
        d = np.abs(np.asarray(u_dev, dtype=np.float64).ravel().astype(LD) - self.u).astype(np.float64)
        b = self.bound_u(E)
        assert np.all(d[b == 0] == 0), "a row whose controls are all zero must come out as exactly zero"
        return float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), 0.0)))


def _weights_ld(costs, lam, shift):
    x = -(np.asarray(costs, dtype=np.float64).astype(LD) - LD(shift)) / LD(lam)
    return np.exp(x), x


def _exact_weight(c, lam, shift, prec):
    import mpmath
    with mpmath.workprec(prec):
        x = -(mpmath.mpf(c) - mpmath.mpf(shift)) / mpmath.mpf(lam)
        w = mpmath.exp(x)
        if w == 0:
            return Fraction(0)
        man, exp = int(w.man), int(w.exp)
        return Fraction(man * 2 ** exp) if exp >= 0 else Fraction(man, 2 ** (-exp))


def _to_ld(fr):
    """Fraction -> longdouble to ~2^-62: numerator and denominator cut to their leading 64 bits, divided, rescaled"""
    if fr == 0:
        return LD(0)
    n, d = abs(fr.numerator), fr.denominator
    bn, bd = max(n.bit_length() - 64, 0), max(d.bit_length() - 64, 0)
    hi = lambda v: LD(v >> 32) * LD(2.0 ** 32) + LD(v & 0xFFFFFFFF)   # (a 64-bit integer, exactly)
    q = np.ldexp(hi(n >> bn) / hi(d >> bd), bn - bd)
    return q if fr > 0 else -q


class Accumulator:
    """S, V, A accumulated over slices of the samples (full sizes: the controls are read back in slices)."""

    def __init__(self, lam, shift=0.0, backend=None):
        self.lam, self.shift = float(lam), float(shift)
        self.backend = backend or ("longdouble" if HAVE_LD64 else "exact80")
        self.K, self.xmax = 0, 0.0
        self.S = self.V = self.A = None

    def add(self, costs, controls):
        costs = np.asarray(costs, dtype=np.float64)
        u = np.asarray(controls, dtype=np.float64).reshape(len(costs), -1)
        self.K += len(costs)
        self.xmax = max(self.xmax, float(np.max(np.abs((costs - self.shift) / self.lam))))
        if self.backend == "longdouble":
            w, _ = _weights_ld(costs, self.lam, self.shift)
            ul = u.astype(LD)
            S, V, A = np.sum(w), np.sum(w[:, None] * ul, axis=0), np.sum(w[:, None] * np.abs(ul), axis=0)
        else:
            prec = 400 if self.backend == "exact" else 80
            w = [_exact_weight(float(c), self.lam, self.shift, prec) for c in costs]
            S = sum(w, Fraction(0))
            uf = [[Fraction(float(v)) for v in row] for row in u]
            V = [sum((w[k] * uf[k][n] for k in range(len(w))), Fraction(0)) for n in range(u.shape[1])]
            A = [sum((w[k] * abs(uf[k][n]) for k in range(len(w))), Fraction(0)) for n in range(u.shape[1])]
        if self.S is None:
            self.S, self.V, self.A = S, V, A
        elif self.backend == "longdouble":
            self.S, self.V, self.A = self.S + S, self.V + V, self.A + A
        else:
            self.S = self.S + S
            self.V = [a + b for a, b in zip(self.V, V)]
            self.A = [a + b for a, b in zip(self.A, A)]
        return self

    def exact_u(self):
        """(exact backends) u_ref as Fractions"""
        return [v / self.S for v in self.V]

    def finish(self):
        if self.backend == "longdouble":
            S, V, A = self.S, self.V, self.A
        else:
            S = _to_ld(self.S)
            V = np.array([_to_ld(v) for v in self.V], dtype=LD)
            A = np.array([_to_ld(a) for a in self.A], dtype=LD)
        return UpdateRef(self.K, self.lam, self.shift, S, V, A, self.xmax)


def reference(costs, controls, lam, shift=0.0, backend=None):
    return Accumulator(lam, shift, backend).add(costs, controls).finish()


# ---- weights ---------------------------------------------------------------------------------------------------------
def weight_errors(costs, lam, w_dev, shift=0.0):
    """(w_ref [K] longdouble, x [K] = -(c - shift)/lambda, |w_dev - w_ref| / (u * w_ref) [K] fp64) for device weights that
    are already multiplied back by sum_w."""
    if HAVE_LD64:
        w, x = _weights_ld(costs, lam, shift)
    else:
        x = -(np.asarray(costs, dtype=np.float64).astype(LD) - LD(shift)) / LD(lam)
        w = np.array([_to_ld(_exact_weight(float(c), lam, shift, 80)) for c in np.asarray(costs, dtype=np.float64)], dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = (np.abs(np.asarray(w_dev, dtype=np.float64).astype(LD) - w) / (LD(U) * w)).astype(np.float64)
    return w, x.astype(np.float64), rel


def measured_exp_ulps(costs, lam, w_dev, shift=0.0):
    """E as the module docstring defines it; the caller asserts E <= E_MAX."""
    w, x, rel = weight_errors(costs, lam, w_dev, shift)
    normal = np.asarray(w > LD(2.0 ** -1000))
    if not normal.any():
        return 1
    k = 2.0 if shift != 0.0 else 1.0
    return max(1, int(math.ceil(float(np.max((rel[normal] - k * np.abs(x[normal]) - 2.0) / 2.0)))))


def check_weights(costs, lam, w_dev, E, shift=0.0):
    """max over k of |w^_k - w_k| / allowed_k  (<= 1 passes); allowed = (|x_k| + 2E + 2) u w_k, floor 2^-1074 (E + 1)."""
    w, x, _ = weight_errors(costs, lam, w_dev, shift)
    k = 2.0 if shift != 0.0 else 1.0
    allowed = np.maximum((LD(k) * np.abs(x).astype(LD) + 2 * E + 2) * LD(U) * w, LD(TINY) * (E + 1))
    return float(np.max(np.abs(np.asarray(w_dev, dtype=np.float64).astype(LD) - w) / allowed))


def zero_count_range(costs, lam, E, shift=0.0):
    """(fewest, most) weights that a correct fp64 evaluation may return as exactly 0 (module docstring: subnormals)."""
    w, x, _ = weight_errors(costs, lam, np.zeros(len(costs)), shift)
    k = 2.0 if shift != 0.0 else 1.0
    rel = (LD(k) * np.abs(x).astype(LD) + 2 * E + 2) * LD(U)
    must = int(np.sum(w * (1 + rel) < LD(TINY) / 2))
    may = int(np.sum(w * (1 - rel) <= LD(TINY)))
    return must, may


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def sensitivities(costs, controls, ref, E=1):
    """(drop [K], swap [K-1]) in units of the rounding bound:
    drop[k] = max_n w_k |u_k[n] - u_ref[n]| / S / bound[n]            what losing sample k moves
    swap[k] = max_n |(w_k - w_{k+1}) (u_k[n] - u_{k+1}[n])| / S / bound[n]   what pairing k's weight with k+1's controls moves
    (rows whose bound is 0 -- a control dimension forced to 0 -- are left out)."""
    costs = np.asarray(costs, dtype=np.float64)
    u = np.asarray(controls, dtype=np.float64).reshape(len(costs), -1)
    w = np.exp(-(costs - ref.shift) / ref.lam)            # fp64 is ample for a ratio that must exceed 100
    b = ref.bound_u(E)
    live = b > 0
    S, ur = float(ref.S), ref.u.astype(np.float64)
    scale = 1.0 / (S * b[live])
    drop = np.max(w[:, None] * np.abs(u[:, live] - ur[live]) * scale, axis=1)
    swap = np.max(np.abs((w[:-1] - w[1:])[:, None] * (u[:-1, live] - u[1:, live])) * scale, axis=1) if len(w) > 1 \
        else np.zeros(0)
    return drop, swap


def sensitivity_ok(drop, swap):
    """the condition on the inputs: every sample's drop sensitivity >= 100, at least 99 % of the neighbour pairs' >= 100"""
    return bool(np.min(drop) >= 100.0 and np.mean(swap >= 100.0) >= 0.99)


def regime_lambda(costs, regime):
    """flat: 1000; graded: (c_max - c_min) / ln 1000, the weights span a factor 1000"""
    if regime == "flat":
        return 1000.0
    if regime == "graded":
        c = np.asarray(costs, dtype=np.float64)
        span = float(c.max() - c.min())
        assert span > 0, "graded regime undefined where c_max == c_min"
        return span / math.log(1000.0)
    raise KeyError(regime)


def fp64_update(costs, controls, lam, shift=0.0):
    """The plain fp64 evaluation, sequential sums (what the oracle does): the subject of the mutation tests."""
    costs = np.asarray(costs, dtype=np.float64)
    u = np.asarray(controls, dtype=np.float64).reshape(len(costs), -1)
    w = np.exp(-(costs - shift) / lam)
    S = 0.0
    V = np.zeros(u.shape[1])
    for k in range(len(w)):
        S += w[k]
        V += w[k] * u[k]
    return V / S, S, w

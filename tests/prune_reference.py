"""The window pruning of the rollout kernels (pc_prune_window, csrc/mppi_consume.h) on the CPU: the specification of the hull
a wave's block of states gets, the ground truth it is judged by, and wrong versions of it.  Needs no GPU
to import.

  device_hull   restates pc_prune_window operation for operation for one wave and one block: the fp32 bounding box of the
                NV x 64 positions (NaN skipped, as v_min_f32 / v_max_f32 skip it), stepped outwards in fp64; f_j at the four
                corners with a correctly rounded fp32 FMA (fmaf32); per lane the better of j = lane and lane + 64 (`upper`), the
                first lane equal to the wave's minimum, jr; da, db, dc, L, T in fp64 without contraction; the keep mask and the
                4-aligned hull [lo & ~3, (hi | 3) + 1) of the survivors.
  exact_nearest the window indices at the smallest TRUE distance of every position, in exact rationals.
  sound         a hull is sound iff for every finite position it contains an index whose fp64 f_j(p) = fma(a, px, fma(b, py, c))
                -- the distance loop's own value, restated with an exact FMA -- equals the minimum over the whole window.  The
                GPU comparison is in bits, so the definition is about the loop's f, not about the true distance: where two
                points' f round to the same double either may stay.  (-0.0 and +0.0 count as equal here: the one window where
                the sign of a zero minimum depends on the order is the one with the pose itself as a window point, and the GPU
                tests compare that one with the switch of the single handle only.)
  WRONG         wrong versions of device_hull, each changing one thing; tests/test_prune_reference.py shows each unsound on at
                least one probe of tests/prune_probe.py, but the two that SOUND names with the reason.

The model is vectorised over the block.  Its fp64 arithmetic is numpy's (IEEE, no contraction); fmaf32 rounds the exact fp64
sum of the exact product and the addend to odd and then to fp32, which is one rounding (53 >= 24 + 2), pinned against rationals
in the test.
"""
import math
from fractions import Fraction

import numpy as np

import obstacle_reference as OR

F32 = np.float32
WRONG = ("box_inwards", "box_states", "box_lanes", "t_negated", "l_ge_t", "t_half", "lo_up", "je_exact", "upper_ignored",
         "upper_half_lost", "nan_in_box")

# The entries of WRONG that are sound all the same: name -> (a probe shows it WASTEFUL -- it keeps more than the specification on
# a probe whose hull the builder promises small --, why no probe built from rollout positions shows it unsound).
SOUND = {
    "upper_ignored": (True, "the inequality holds against ANY window point r; taking `lane` where `lane + 64` was the better "
                            "candidate only gives a worse dominator: fewer points are dropped, none wrongly"),
    "t_half": (False, "T guards the roundings of L and of the loop's f, which are below 1e-15 of the sum of magnitudes; what "
                      "decides a near case is the outward step of the box, 1.2e-7 |edge|, nine orders above them, and it enters "
                      "L, not T: with half of T, or with T = 0, the same points are dropped on every probe built from a rollout's "
                      "positions (there the step vanishes only for an edge at exactly 0, attained by the pose's own state 0, "
                      "where f_j = c_j is exact).  This is an observation about such probes, not a theorem: a crafted block with "
                      "a binding edge at a tiny non-zero coordinate would leave T alone to cover the roundings; none is built"),
}


def h4_of(H):
    return (int(H) + 3) & ~3


def window_coeffs(xr, yr, x0=(0.0, 0.0)):
    """a, b, c as window_coeffs() (ccv_mppi_capi.hip) forms them: plain fp64, no contraction"""
    with np.errstate(all="ignore"):
        xl = np.asarray(xr, dtype=np.float64) - np.float64(x0[0])
        yl = np.asarray(yr, dtype=np.float64) - np.float64(x0[1])
        return -2.0 * xl, -2.0 * yl, xl * xl + yl * yl


# ---- fp32 FMA with one rounding ----------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product of two fp32 numbers is exact in fp64; its sum with c is formed with its
    error (two-sum), forced to an odd last bit where the error is not zero, and rounded to fp32"""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        bits = np.ascontiguousarray(s).view(np.int64).copy()
        even = (bits & 1) == 0
        # towards the error: for a positive s a larger magnitude is the next integer up, for a negative s too (sign-magnitude)
        up = (err > 0.0) == (s > 0.0)
        bits = np.where(fix & even, np.where(up, bits + 1, bits - 1), bits)
        # (s == 0 with err != 0 cannot happen: then p = -c exactly)
        return bits.view(np.float64).astype(F32)


def fmaf32_rational(a, b, c):
    """the same for three finite fp32 scalars through exact rationals (one rounding: to the nearest fp32, ties to even)"""
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if r == 0:
        return F32(0.0)
    d = float(r)          # correctly rounded to fp64: only a first guess
    lo = hi = F32(d)
    if Fraction(float(lo)) > r:
        lo = np.nextafter(lo, F32(-np.inf))
    else:
        hi = np.nextafter(lo, F32(np.inf)) if Fraction(float(lo)) < r else lo
    if lo == hi:
        return lo
    dl, dh = r - Fraction(float(lo)), Fraction(float(hi)) - r
    if dl != dh:
        return lo if dl < dh else hi
    return lo if (int(np.array(lo).view(np.int32)) & 1) == 0 else hi


def fmaf32_detour(a, b, c):
    """what fmaf32 must not be: the fp64 sum cast to fp32 (two roundings)"""
    with np.errstate(all="ignore"):
        return F32(np.float64(a) * np.float64(b) + np.float64(c))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _last_nan_min(v, sign):
    """a minimum (sign = 1) or maximum (-1) written as `lo = lo < x ? lo : x`: a NaN replaces what was found before it"""
    v = np.asarray(v, dtype=F32).ravel() * F32(sign)
    nan = np.flatnonzero(np.isnan(v))
    if len(nan) and nan[-1] == len(v) - 1:
        return F32(np.nan)
    tail = v[nan[-1] + 1:] if len(nan) else v
    return F32(tail.min() * F32(sign))


def device_hull(px, py, a, b, c, H, wrong=None):
    """(jb, je, keep [H4] bool, jr [4]) of one wave's block: px, py [NV][64] float64 relative to the pose, a, b, c [H] float64"""
    assert wrong is None or wrong in WRONG, "unknown wrong version %r" % (wrong,)
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    assert px.ndim == 2 and px.shape[1] == 64 and px.shape == py.shape, "positions are [NV][64]"
    H, H4 = int(H), h4_of(H)
    nhalf = 2 if H4 > 64 else 1
    with np.errstate(all="ignore"):
        fx, fy = px.astype(F32), py.astype(F32)
        if wrong == "box_states" and fx.shape[0] > 1:
            fx, fy = fx[:-1], fy[:-1]
        if wrong == "box_lanes":
            fx, fy = fx[:, :63], fy[:, :63]
        if wrong == "nan_in_box":
            xlo, xhi, ylo, yhi = _last_nan_min(fx, 1), _last_nan_min(fx, -1), _last_nan_min(fy, 1), _last_nan_min(fy, -1)
        else:   # fminf / v_min_f32: the number of a number and a NaN
            xlo, xhi, ylo, yhi = np.fmin.reduce(fx, axis=None), np.fmax.reduce(fx, axis=None), np.fmin.reduce(fy, axis=None), np.fmax.reduce(fy, axis=None)
        xlo, xhi, ylo, yhi = F32(xlo), F32(xhi), F32(ylo), F32(yhi)
        step = (lambda v: 0.0) if wrong == "box_inwards" else (lambda v: abs(np.float64(v)) * 1.2e-7 + 1.0e-37)
        bx0, bx1 = np.float64(xlo) - step(xlo), np.float64(xhi) + step(xhi)
        by0, by1 = np.float64(ylo) - step(ylo), np.float64(yhi) + step(yhi)
        X, Y = np.fmax(abs(bx0), abs(bx1)), np.fmax(abs(by0), abs(by1))
        # this lane's window points
        j = np.arange(64)[None, :] + 64 * np.arange(nhalf)[:, None]                 # [nhalf][64]
        valid = j < H
        jj = np.where(valid, j, 0)
        A = np.where(valid, np.asarray(a, dtype=np.float64)[jj], 0.0)
        B = np.where(valid, np.asarray(b, dtype=np.float64)[jj], 0.0)
        Cc = np.where(valid, np.asarray(c, dtype=np.float64)[jj], np.inf)
        tj = 1.0e-9 * (np.abs(Cc) + (np.abs(A) * X + np.abs(B) * Y))
        a32, b32, c32 = A.astype(F32), B.astype(F32), Cc.astype(F32)
        corners = ((xlo, ylo), (xlo, yhi), (xhi, ylo), (xhi, yhi))
        v = [fmaf32(a32, np.full_like(a32, cx), fmaf32(b32, np.full_like(a32, cy), c32)) for cx, cy in corners]   # 4 x [nhalf][64]
        jr, ok, Ar, Br, Cr = [], [], [], [], []
        for k in range(4):
            mine, upper = v[k][0], np.zeros(64, dtype=bool)
            if nhalf == 2 and wrong != "upper_half_lost":
                upper = v[k][1] < v[k][0]
                mine = np.where(upper, v[k][1], v[k][0])
            best = np.fmin.reduce(mine)
            at = np.flatnonzero(mine == best)
            ok.append(len(at) > 0)
            r = int(at[0]) if len(at) else 0
            jr.append(r + (64 if (upper[r] and wrong != "upper_ignored") else 0))
            # jr >= H: every valid lane's value is NaN and the first padding lane's +inf is the minimum (a window of points beyond
            # fp32's range).  The device reads the padding there, a = b = 0, c = +inf, against which nothing is dropped (for H a
            # multiple of four and below 64 it reads the entry after the padding, which nothing stages: DESIGN.md section 13)
            pad = jr[k] >= H
            Ar.append(np.float64(0.0 if pad else np.asarray(a, dtype=np.float64)[jr[k]]))
            Br.append(np.float64(0.0 if pad else np.asarray(b, dtype=np.float64)[jr[k]]))
            Cr.append(np.float64(np.inf if pad else np.asarray(c, dtype=np.float64)[jr[k]]))
        kp = valid.copy()
        for k in range(4):
            da, db, dc = A - Ar[k], B - Br[k], Cc - Cr[k]
            L = dc + (np.fmin(da * bx0, da * bx1) + np.fmin(db * by0, db * by1))
            tr = 1.0e-9 * (abs(Cr[k]) + (abs(Ar[k]) * X + abs(Br[k]) * Y))
            T = tj if wrong == "t_half" else tj + tr
            if wrong == "t_negated":
                T = -T
            dominated = (L >= T) if wrong == "l_ge_t" else (L > T)
            kp = kp & ~(ok[k] & dominated)
        if wrong == "upper_half_lost" and nhalf == 2:
            kp[1] = False
    keep = kp.ravel()[:H4].copy()   # (j = lane + 64 hh; H4 <= 64 nhalf)
    jb, je = 0, H4
    if keep.any():
        idx = np.flatnonzero(keep)
        lo, hi = int(idx[0]), int(idx[-1])
        jb = ((lo + 3) & ~3) if wrong == "lo_up" else (lo & ~3)
        je = hi + 1 if wrong == "je_exact" else (hi | 3) + 1
    return jb, je, keep, jr


def switch_trace(blocks, a, b, c, H, wrong=None):
    """the hulls of one wave over a launch, with the prune_on switch of pc_consume: `blocks` is a list of (px, py) in block
    order; once a block keeps more than 3/4 of the padded window the wave stops testing.  -> a list of (jb, je, tested)"""
    H4, on, out = h4_of(H), True, []
    for px, py in blocks:
        if not on:
            out.append((0, H4, False))
            continue
        jb, je, _, _ = device_hull(px, py, a, b, c, H, wrong)
        if 4 * (je - jb) > 3 * H4:
            on = False
        out.append((jb, je, True))
    return out


# ---- the ground truth ----------------------------------------------------------------------------------------------------------
def loop_f(a, b, c, x, y):
    """the distance loop's f_j(p) = fma(a, px, fma(b, py, c)) for scalars, with an exact FMA"""
    return OR.fma(a, x, OR.fma(b, y, c))


def _approx(px, py, a, b, c):
    """(F, tol) [N][H]: f in plain fp64 and a bound of its distance from the loop's value (two roundings of each, and a dropped
    product error: 4 u of the magnitudes covers them with room); NaN -> +inf with tol 0 (fmin drops a NaN)"""
    with np.errstate(all="ignore"):
        ax, by = a[None, :] * px[:, None], b[None, :] * py[:, None]
        F = ax + (by + c[None, :])
        S = np.abs(ax) + np.abs(by) + np.abs(c)[None, :]
        tol = np.where(np.isfinite(S), 4.0 * 2.0 ** -52 * S, 0.0)
        F = np.where(np.isnan(F), np.inf, F)
    return F, tol


def loop_minimum(px, py, a, b, c, H, hull=None):
    """per finite position (flattened [N]) the minimum of the loop's f over window indices [jb, je) n [0, H) -- every index
    without `hull` -- as fmin leaves it (a NaN is dropped; +inf when nothing is left), exact: candidates by _approx, the
    decision among them by loop_f"""
    px, py = np.asarray(px, dtype=np.float64).ravel(), np.asarray(py, dtype=np.float64).ravel()
    a, b, c = (np.asarray(v, dtype=np.float64)[:H] for v in (a, b, c))
    jb, je = (0, H) if hull is None else (max(int(hull[0]), 0), min(int(hull[1]), H))
    out = np.full(len(px), np.inf)
    if je <= jb:
        return out
    F, tol = _approx(px, py, a[jb:je], b[jb:je], c[jb:je])
    with np.errstate(all="ignore"):
        upper = np.min(F + tol, axis=1)
        cand = (F - tol) <= upper[:, None]
    for i in range(len(px)):
        if not (math.isfinite(px[i]) and math.isfinite(py[i])):
            out[i] = np.nan
            continue
        js = np.flatnonzero(cand[i])
        m = math.inf
        for j in js:
            m = OR.fmin(m, loop_f(a[jb + j], b[jb + j], c[jb + j], px[i], py[i]))
        out[i] = m
    return out


def sound(hull, px, py, a, b, c, H, full=None):
    """the hull (jb, je) is one the distance loop takes -- 4-aligned, not empty, inside the padded window (the loop starts from
    its first pair of points and runs in fours: pc_consume) -- and holds, for every finite position, an index whose loop value equals the minimum over the whole window
    (module docstring).  -> (bool, the flattened positions where it does not); `full`: loop_minimum over the whole window, when
    the caller has it"""
    jb, je = int(hull[0]), int(hull[1])
    if not (0 <= jb < je <= h4_of(H) and jb % 4 == 0 and (je - jb) % 4 == 0):
        return False, np.arange(0)   # not a hull the loop takes: it starts at a multiple of four and runs in fours
    if full is None:
        full = loop_minimum(px, py, a, b, c, H)
    part = loop_minimum(px, py, a, b, c, H, hull)
    fin = ~np.isnan(full)
    bad = np.flatnonzero(fin & ~(part == full))
    return len(bad) == 0, bad


def exact_nearest(px, py, xr, yr):
    """for every position (flattened) the list of the window indices at the smallest true distance, in exact rationals; [] for
    a position that is not finite; window points that are not finite are never nearest"""
    px, py = np.asarray(px, dtype=np.float64).ravel(), np.asarray(py, dtype=np.float64).ravel()
    xr, yr = np.asarray(xr, dtype=np.float64), np.asarray(yr, dtype=np.float64)
    ok = np.isfinite(xr) & np.isfinite(yr)
    with np.errstate(all="ignore"):
        dx, dy = px[:, None] - xr[None, :], py[:, None] - yr[None, :]
        D = np.where(ok[None, :], dx * dx + dy * dy, np.inf)
        D = np.where(np.isnan(D), np.inf, D)
        cand = D <= np.min(D, axis=1)[:, None] * (1.0 + 1.0e-12)
    out = []
    for i in range(len(px)):
        if not (math.isfinite(px[i]) and math.isfinite(py[i])) or not ok.any():
            out.append([])
            continue
        js = [int(j) for j in np.flatnonzero(cand[i] & ok)]
        if len(js) > 1:
            fx, fy = Fraction(px[i]), Fraction(py[i])
            d = [(fx - Fraction(xr[j])) ** 2 + (fy - Fraction(yr[j])) ** 2 for j in js]
            js = [j for j, dj in zip(js, d) if dj == min(d)]
        out.append(js)
    return out

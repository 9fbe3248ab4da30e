"""Windows that put the window pruning of the rollout kernels (pc_prune_window) on its edges, built from the positions of one
wave's block of states -- the device's own, read back, or a synthetic fan's.  Needs no GPU to import.

Every builder takes px, py [NV][64] (relative to the pose; the GPU tests put the pose at the origin) and returns a Probe: the
window xr, yr, the index j of the LIVE point, the index r of the dominator it was built against, the flattened index of the
position p* the live point is nearest to, and the facts it promises, each asserted here with exact arithmetic
(prune_reference.loop_f / exact_nearest), so that a block that cannot carry the probe fails as a condition, not as a finding.

  ladder     p* is the position that alone attains one edge of the block's bounding box (xhi, xlo, yhi, ylo in turn).  The
             dominator r lies t behind p* along the edge's normal, the live point r_j about t in front of it, so that their
             bisector cuts off p* alone: f_r(p*) - f_j(p*) = eps > 0 in the loop's own fp64 f, every other position is nearer
             to r.  eps is 2^k ulps, k = 2, 4, .., 30, of the larger of p*'s d^2 and |p*|^2: f = d^2 - |p|^2, so
             where a sample is farther from the pose than from the window, no margin below an ulp of |p|^2 exists (r_j's
             coordinate along the normal is moved ulp by ulp, then r_j sideways by eta, which takes eta^2 off the margin, until
             the loop's margin is within a factor 4 of eps).
             Removing j changes the bits of p*'s d^2 (asserted): the probe is live.  Every other window point lies far behind
             r; r is given twice (slot r and the slot the caller names `twin`), which is what lets permuted() below find two
             survivors.
  fp32_gap   the same with the bisector strictly between fl32(edge) and the edge, for a block whose edge rounds inwards in
             fp32 (about half of them do): p* lies outside the fp32 box, and only the outward step keeps j.  t is searched
             until the model does not choose j as a dominator itself (a dominator is kept whatever the box is).
  edges      a ladder rung (k = 10) with the live point and the dominator at given indices: 0, 1, 3, 4, 62, 63, 64, 65, H - 2,
             H - 1 in turn for each; two_live() with the live point given twice, at 1 and H - 2, and a dead middle; the single
             survivor.
  degenerate a window point exactly at the pose (a = b = c = 0, so T = 0) given three times; a fan whose 64 lanes coincide
             (coincident() on the CPU, a launch without noise on the device), with on_states(): window points on the very
             positions that are the box's edges; a position exactly 0.
  permuted   the same points in an order with two survivors of every tested block at indices 0 and H - 1: there the model's
             hull is [0, H4) for every block (asserted by the caller's switch trace), so this order IS the full loop for a
             kernel that has no switch.  fmin over the same values in another order gives the same bits -- fmin is
             commutative and associative on numbers, a NaN is dropped in any order -- so the costs of the two orders must be
             equal in every bit, and the batch kernels need no twin without pruning.  The one exception is a minimum that is a
             zero of either sign (fmin(+0, -0) depends on the order): only the window with the pose itself as a point has one,
             and that window is compared through CCV_MPPI_PRUNE on the single handle only.
"""
import math
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np

import prune_reference as PR

Probe = namedtuple("Probe", "xr yr j r star margin eps what")
SIDES = ("xhi", "xlo", "yhi", "ylo")
RUNGS = tuple(range(2, 31, 2))
EXACT_FROM = 8        # rungs from 2^8 ulps on: the margin is beyond the roundings of f (a few ulps), the true distances agree
EDGE_SLOTS = (0, 1, 3, 4, 62, 63, 64, 65, -2, -1)
T_LIST = (0.5, 0.8, 1.3, 0.35, 2.1, 0.6, 1.0, 1.7, 0.45, 2.9, 0.7, 1.1)


# ---- synthetic fans --------------------------------------------------------------------------------------------------------
def synthetic_fan(seed, T, lanes=64, v=0.6, dt=0.1, noise=0.8, heading=0.3):
    """states [lanes][T][2] of a diff-drive rollout of random controls from the origin (numpy's generator: nothing of the
    device's noise stream)"""
    rng = np.random.default_rng(seed)
    speed = np.clip(v + 0.2 * rng.standard_normal((lanes, T - 1)), 0.05, 1.2)
    omega = noise * rng.standard_normal((lanes, T - 1))
    P, th = np.zeros((lanes, T, 2)), np.full(lanes, heading)
    for k in range(T - 1):
        P[:, k + 1, 0] = P[:, k, 0] + speed[:, k] * np.cos(th) * dt
        P[:, k + 1, 1] = P[:, k, 1] + speed[:, k] * np.sin(th) * dt
        th = th + omega[:, k] * dt
    return P


def block_of(P, b, nstates=None):
    """(px, py) [NV][64] of block b (states 8 b .. 8 b + NV - 1) of the wave's states P [64][T][2]"""
    T = P.shape[1] if nstates is None else nstates
    nv = min(8, T - 8 * b)
    assert nv >= 1 and P.shape[0] == 64, "no such block: b = %d of %d states, %d lanes" % (b, T, P.shape[0])
    return P[:, 8 * b:8 * b + nv, 0].T.copy(), P[:, 8 * b:8 * b + nv, 1].T.copy()


def blocks_of(P, nstates=None):
    T = P.shape[1] if nstates is None else nstates
    return [block_of(P, b, T) for b in range((T + 7) // 8)]


# ---- pieces ------------------------------------------------------------------------------------------------------------------
def _axis(side):
    return (0 if side[0] == "x" else 1), (1.0 if side.endswith("hi") else -1.0)


def extreme(px, py, side):
    """(flattened index of the position that alone attains the edge, its gap to the next one along the normal); None where two
    positions share the edge"""
    ax, sg = _axis(side)
    s = sg * (px if ax == 0 else py).ravel()
    order = np.argsort(-s)
    gap = float(s[order[0]] - s[order[1]])
    return (int(order[0]), gap) if gap > 0.0 else None


def d2_bits(f_min, x, y):
    """the bits of the kernel's d^2 = m + fma(px, px, py py) for a minimum m"""
    return np.float64(f_min + PR.OR.fma(x, x, y * y)).view(np.uint64)


def _slot(s, H):
    return s % H


def _fill(H, r_xy, normal, depth, slots, points):
    """a window of H points: `points` at `slots`, every other one far behind r along -normal, each a little farther"""
    xr, yr = np.zeros(H), np.zeros(H)
    free = [i for i in range(H) if i not in slots]
    for n, i in enumerate(free):
        back = depth * (1.0 + 0.01 * n)
        xr[i] = r_xy[0] - back * normal[0] + 0.003 * (n % 7) * normal[1]
        yr[i] = r_xy[1] - back * normal[1] + 0.003 * (n % 7) * normal[0]
    for i, (x, y) in zip(slots, points):
        xr[i], yr[i] = x, y
    return xr, yr


def _margin(xr, yr, j, r, x, y):
    a, b, c = PR.window_coeffs(xr, yr)
    return PR.loop_f(a[r], b[r], c[r], x, y) - PR.loop_f(a[j], b[j], c[j], x, y)


def promises(what, px, py, xr, yr, j, star, exact=True):
    """asserted for every probe with a live point: in the loop's f it is the strict minimum at p*, and without it the bits of
    p*'s d^2 change; with `exact` (every probe but the ladder's rungs below EXACT_FROM, whose margin lies inside the rounding
    of f, so that the true distances may order the other way) also in exact rationals: j alone is nearest to p*, and to no other
    position (but the positions equal to p*)"""
    H = len(xr)
    x, y = float(px.ravel()[star]), float(py.ravel()[star])
    if exact:
        near = PR.exact_nearest(px, py, xr, yr)
        assert near[star] == [j], "%s: the live point %d is not alone nearest to p* (%s)" % (what, j, near[star])
        same = (px.ravel() == x) & (py.ravel() == y)
        taken = [i for i, js in enumerate(near) if j in js and not same[i]]
        assert not taken, "%s: the live point is nearest to other positions too: %s" % (what, taken[:6])
    a, b, c = PR.window_coeffs(xr, yr)
    f = [PR.loop_f(a[m], b[m], c[m], x, y) for m in range(H)]
    rest = min(f[m] for m in range(H) if m != j)
    assert f[j] < rest, "%s: the loop's f_j(p*) is not the strict minimum (%r against %r)" % (what, f[j], rest)
    assert d2_bits(f[j], x, y) != d2_bits(rest, x, y), "%s: removing the live point leaves the bits of d^2: the probe is dead" % what
    return rest - f[j]


# ---- the bisector ladder ---------------------------------------------------------------------------------------------------------
def ladder(px, py, H, side, k, t=0.5, j=None, r=None, twin=None, delta=None, check=True):
    """the rung k of the ladder on the edge `side` (module docstring); delta: the distance of the bisector inside p* given
    directly (fp32_gap), eps then follows from it"""
    ax, sg = _axis(side)
    got = extreme(px, py, side)
    assert got is not None, "ladder %s: two positions share the edge" % side
    star, gap = got
    x, y = float(px.ravel()[star]), float(py.ravel()[star])
    normal = (sg, 0.0) if ax == 0 else (0.0, sg)
    r = ((H // 2) & ~3) + 1 if r is None else _slot(r, H)   # (defaults: the live point in another group of four than r)
    j = (r + 5) % H if j is None else _slot(j, H)
    twin = next(s % H for s in (r + 1, r + 2, r + 3) if s % H != j) if twin is None else _slot(twin, H)
    assert len({j, r, twin}) == 3, "ladder: the live point, the dominator and its twin need three slots"
    # the margin is a difference of two f = d^2 - |p|^2: it moves in ulps of the larger of d^2 (= t^2) and |p*|^2
    ulp = math.ulp(max(t * t, x * x + y * y))
    eps = None if delta is not None else (2.0 ** k) * ulp
    dl = delta if delta is not None else eps / (4.0 * t)
    assert dl < 0.5 * gap, "ladder %s k=%s: the bisector would cut off a second position (delta %.3g, gap %.3g)" % (side, k, dl, gap)
    star_s = x if ax == 0 else y
    rs, js = star_s - sg * (t + dl), star_s + sg * (t - dl)
    extent = float(np.ptp(px if ax == 0 else py)) + t
    r_xy = (rs, y) if ax == 0 else (x, rs)

    def window(js_, side_step=0.0):
        j_xy = (js_, y + side_step) if ax == 0 else (x + side_step, js_)
        return _fill(H, r_xy, normal, 2.0 * extent + 2.0, [r, twin, j], [r_xy, r_xy, j_xy])

    xr, yr = window(js)
    m = _margin(xr, yr, j, r, x, y)
    if eps is not None:
        # r_j's coordinate along the normal ulp by ulp towards p* until the margin is eps or more (one ulp is worth some ulps
        # of d^2), then r_j sideways by eta: that takes eta^2 off the margin, as fine as needed
        for _ in range(400):
            if m >= eps:
                break
            js = float(np.nextafter(js, -sg * math.inf))
            xr, yr = window(js)
            m = _margin(xr, yr, j, r, x, y)
        if m > eps:
            eta = math.sqrt(m - eps)
            best = (abs(m - eps), xr, yr, m)
            for f in (1.0, 0.98, 1.02, 0.95, 1.05, 0.9):
                xr2, yr2 = window(js, f * eta)
                m2 = _margin(xr2, yr2, j, r, x, y)
                if m2 > 0.0 and abs(m2 - eps) < best[0]:
                    best = (abs(m2 - eps), xr2, yr2, m2)
            _, xr, yr, m = best
        assert 0.25 * eps <= m <= 4.0 * eps, "ladder %s k=%d: no margin within a factor 4 of eps = %.3g (last %.3g)" % (side, k, eps, m)
    what = "ladder %s k=%s t=%g j=%d r=%d" % (side, k, t, j, r)
    if check:
        m2 = promises(what, px, py, xr, yr, j, star, exact=k is None or k >= EXACT_FROM)
        assert m2 == m, "%s: the dominator is not the runner-up (%r against %r)" % (what, m2, m)
    return Probe(xr, yr, j, r, star, m, eps if eps is not None else m, what)


def fp32_rounds_inwards(px, py, side):
    """the edge of the block, attained by one position alone, lies outside the fp32 box before its outward step"""
    ax, sg = _axis(side)
    got = extreme(px, py, side)
    if got is None:
        return False
    v = float((px if ax == 0 else py).ravel()[got[0]])
    return sg * float(np.float32(v)) < sg * v


def fp32_gap(px, py, H, side):
    """the bisector strictly between fl32(edge) and the edge; t searched until the model does not choose j as a dominator and
    the model WITHOUT the outward step drops j (promised: the probe is one that only the step holds)"""
    ax, sg = _axis(side)
    assert fp32_rounds_inwards(px, py, side), "fp32 gap %s: the edge does not round inwards" % side
    star, gap = extreme(px, py, side)
    v = float((px if ax == 0 else py).ravel()[star])
    width = abs(v - float(np.float32(v)))
    for t in T_LIST:
        if 0.5 * width >= 0.5 * gap:
            break
        p = ladder(px, py, H, side, None, t=t, delta=0.5 * width, check=False)
        a, b, c = PR.window_coeffs(p.xr, p.yr)
        _, _, keep, jr = PR.device_hull(px, py, a, b, c, H)
        if p.j in jr:
            continue
        if PR.device_hull(px, py, a, b, c, H, "box_inwards")[2][p.j]:
            continue   # (the gap is too narrow at this t: L stays below T even without the step, the probe would prove nothing)
        # the promise, in exact rationals: fl32(edge) < bisector < edge along the normal
        coord = p.xr if ax == 0 else p.yr
        bis = (Fr(float(coord[p.r])) + Fr(float(coord[p.j]))) / 2
        lo, hi = sorted((Fr(float(np.float32(v))), Fr(v)))
        assert lo < bis < hi, "fp32 gap %s: the bisector is not inside the gap" % side
        promises("fp32 gap %s t=%g" % (side, t), px, py, p.xr, p.yr, p.j, star)
        return p._replace(what="fp32 gap %s t=%g" % (side, t))
    raise AssertionError("fp32 gap %s: for every t tried the model chooses the live point as a dominator, or keeps it without the "
                         "outward step as well" % side)


# ---- hull edges --------------------------------------------------------------------------------------------------------------
def edge_cases(H):
    """(j, r, twin) slots: the live point at each edge slot with the dominator mid-window, then the dominator at each with the
    live point mid-window"""
    slots = sorted({_slot(s, H) for s in EDGE_SLOTS if -H <= s < H})
    mid = H // 2 if H // 2 not in slots and H // 2 + 1 not in slots else H // 2 + 5
    out = [(s, mid, mid + 1) for s in slots] + [(mid, s, mid + 1) for s in slots]
    return [c for c in out if len(set(c)) == 3]


def edge(px, py, H, j, r, twin, side="xhi"):
    return ladder(px, py, H, side, 10, j=j, r=r, twin=twin)


def two_live(px, py, H):
    """two live points far apart in index (1 and H - 2: the rung k = 10 on xhi, its live point given twice), the dominator and
    its twin mid-window, everything else dead: the hull spans the dead middle.  Either copy alone keeps p*'s bits; the pair is
    live (asserted: without both, the bits of d^2 change).  The copies being equal, a hull that lost ONE of them gives the same
    costs: this case shows a hull over a dead middle running, not that both clusters are held -- the edge cases do that, with the
    live point at 0 or H - 1 and the dominator, which other positions need, mid-window.  -> (Probe, the second live index)"""
    p = ladder(px, py, H, "xhi", 10, j=1, check=False)
    j2 = H - 2
    assert j2 not in (p.r, p.j) and (p.xr[j2], p.yr[j2]) != (p.xr[p.r], p.yr[p.r]), "two live: slot H - 2 is taken"
    xr, yr = p.xr.copy(), p.yr.copy()
    xr[j2], yr[j2] = xr[1], yr[1]
    x, y = float(px.ravel()[p.star]), float(py.ravel()[p.star])
    a, b, c = PR.window_coeffs(xr, yr)
    f = [PR.loop_f(a[m], b[m], c[m], x, y) for m in range(H)]
    rest = min(f[m] for m in range(H) if m not in (1, j2))
    assert f[1] == f[j2] < rest, "two live: the pair is not the strict minimum at p*"
    assert d2_bits(f[1], x, y) != d2_bits(rest, x, y), "two live: removing the pair leaves the bits of d^2"
    return Probe(xr, yr, 1, p.r, p.star, rest - f[1], p.eps, "two live points (1, %d)" % j2), j2


def single_survivor(px, py, H, slot=None, twin=False):
    """one point in front of everything, every other far behind it: the model keeps it alone; twin: given twice, five slots
    apart (two survivors, for permuted())"""
    slot = H // 2 + 1 if slot is None else _slot(slot, H)
    cx, cy = float(np.mean(px)), float(np.mean(py))
    slots = [slot, (slot + 5) % H] if twin else [slot]
    xr, yr = _fill(H, (cx, cy), (1.0, 0.0), 2.0 * float(np.ptp(px)) + 2.0 * float(np.ptp(py)) + 3.0, slots, [(cx, cy)] * len(slots))
    return Probe(xr, yr, slot, slot, 0, math.inf, math.inf, "%s survivor at %d" % ("twin" if twin else "single", slot))


def on_states(px, py, H, slots=(5, 13, 6)):
    """window points exactly ON lane 0's first and last state of the block (d^2 = 0 there; one state: the same point) and the
    first once more (two survivors wherever it is a dominator, for permuted()), the rest far behind: for a block whose lanes coincide the box's edges are these very positions, and only the outward step lies
    between the box and them"""
    pts = [(float(px[0, 0]), float(py[0, 0])), (float(px[-1, 0]), float(py[-1, 0]))]
    way = (pts[1][0] - pts[0][0], pts[1][1] - pts[0][1])
    n = math.hypot(*way)
    normal = (way[0] / n, way[1] / n) if n > 0.0 else (1.0, 0.0)
    xr, yr = _fill(H, pts[0], normal, 2.0 * float(np.ptp(px)) + 2.0 * float(np.ptp(py)) + 3.0, list(slots), pts + pts[:1])
    return Probe(xr, yr, slots[1], slots[0], px.size - 64, math.inf, math.inf, "on the block's first and last state")


# ---- degenerate --------------------------------------------------------------------------------------------------------------
def pose_point(px, py, H, slots=(5, 6, 7), other=13):
    """the pose itself as a window point, three times (a = b = c = 0: T = 0 against itself); one more point on the position
    farthest from the pose, in another group of four (it survives too: a hull of the survivors that lost the pose's copies
    would not hold them); the rest far away"""
    far = int(np.argmax(np.nan_to_num(px.ravel() ** 2 + py.ravel() ** 2, nan=-1.0, posinf=-1.0)))
    q = (float(px.ravel()[far]), float(py.ravel()[far]))
    xr, yr = _fill(H, (0.0, 0.0), (1.0, 0.0), 50.0, list(slots) + [other], [(0.0, 0.0)] * len(slots) + [q])
    return Probe(xr, yr, slots[0], slots[0], far, math.inf, math.inf, "pose point x%d" % len(slots))


def coincident(px, py):
    """the block with all 64 lanes on lane 0's states (a zero-noise run)"""
    return np.repeat(px[:, :1], 64, axis=1), np.repeat(py[:, :1], 64, axis=1)


# ---- permutation pairs ---------------------------------------------------------------------------------------------------------
def permuted(xr, yr, first_blocks, H):
    """(xr, yr, order) with two points that survive each of `first_blocks` (the first block of every wave: a list of (px, py))
    at indices 0 and H - 1; order[i] is the index the new point i had.  The caller asserts by prune_reference.switch_trace that
    the model's hull is [0, H4) for every block of every wave in this order."""
    a, b, c = PR.window_coeffs(xr, yr)
    keep = np.ones(PR.h4_of(H), dtype=bool)
    for px, py in first_blocks:
        keep &= PR.device_hull(px, py, a, b, c, H)[2]
    alive = [int(i) for i in np.flatnonzero(keep[:H])]
    assert len(alive) >= 2, "permuted: fewer than two points survive the first block of every wave (%s)" % alive
    i0, i1 = alive[0], alive[-1]
    order = list(range(H))
    order[0], order[i0] = order[i0], order[0]
    k = order.index(i1)
    order[H - 1], order[k] = order[k], order[H - 1]
    order = np.array(order)
    assert sorted(order) == list(range(H)), "permuted: not a permutation"
    return np.asarray(xr)[order], np.asarray(yr)[order], order

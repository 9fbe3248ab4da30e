"""The fleets that hold the fleet term's selection at its edges: the cases that
tests/test_fleet_reference.py pins on the CPU between the two backends of tests/fleet_reference.py and that
tests/test_gpu_batch_fleet_edges.py runs through the six prologue kernels, and the wrong versions of the selection that must each
differ on one of them.

A case is a dict: q [B][2] the positions the selection is formed on, radius [B], n_static [B], maxn (max_neighbours), rng
(range), q_post [B][2] (positions after an advance, for the wrong version that takes them as the centre), finite (False: the
float64 backend only), q_next (a second position set for the same handle, or None) and info (what the seeded search that built
the case found; the CPU test asserts the case's condition from it and from the positions).  Every search is seeded and takes
well under a second.  No test and no fixture lives here; imports fleet_reference only.
"""
from fractions import Fraction

import numpy as np

import fleet_reference as FR

KBLOCK = 256   # the prologue workgroup's width: robot j is candidate j // 256 of thread j % 256, in wave (j % 256) // 64


def _case(name, q, radius, n_static, max_neighbours, rng, q_post=None, finite=True, q_next=None, info=None):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
    B = len(q)
    q_post = q + np.array([0.013, -0.007]) * (1 + np.arange(B))[:, None] if q_post is None else np.asarray(q_post, dtype=np.float64)
    return dict(name=name, q=q, q_post=q_post, radius=np.broadcast_to(np.asarray(radius, dtype=np.float64), (B,)).copy(),
                n_static=np.broadcast_to(np.asarray(n_static, dtype=np.int32), (B,)).copy(), maxn=int(max_neighbours), rng=float(rng),
                finite=bool(finite), q_next=None if q_next is None else np.asarray(q_next, dtype=np.float64).reshape(B, 2),
                info=info or {})


def args(c, q=None):
    """the case as fleet_reference.lists takes it, on q (default: the case's first positions)"""
    return (c["q"] if q is None else q, c["radius"], c["n_static"], c["maxn"], c["rng"])


def positions(c):
    """the position sets a handle is given in turn"""
    return [c["q"]] if c["q_next"] is None else [c["q"], c["q_next"]]


# ---- d2 in the spec's form and in the two contracted forms -----------------------------------------------------------------
def d2_forms(qj, qy):
    """(dx*dx + dy*dy, fma(dx, dx, dy*dy), fma(dy, dy, dx*dx)) of robot j seen from robot y as doubles, from exact rationals
    rounded after every operation (fleet_reference._rd); an FMA is the exact product plus the addend, rounded once"""
    F, rd = Fraction, FR._rd
    dx = rd(F(float(qj[0])) - F(float(qy[0])))
    dy = rd(F(float(qj[1])) - F(float(qy[1])))
    xx, yy = dx * dx, dy * dy
    return float(rd(rd(xx) + rd(yy))), float(rd(xx + rd(yy))), float(rd(yy + rd(xx)))


def _product_is_exact(a):
    """a * a has no rounding error (Dekker's product on Veltkamp's split; a finite and far from over- and underflow)"""
    p = a * a
    t = 134217729.0 * a
    hi = t - (t - a)
    lo = a - hi
    return ((hi * hi - p) + 2.0 * hi * lo) + lo * lo == 0.0


def d2_contracted(dx, dy):
    """fma(dx, dx, dy * dy) for float64 arrays.  Where dx * dx is exact the contraction changes nothing; elsewhere the FMA is
    taken from exact rationals.  Where a value is not finite both forms give the same infinity or NaN."""
    with np.errstate(all="ignore"):
        yy = dy * dy
        out = dx * dx + yy
        fin = np.isfinite(dx) & np.isfinite(yy) & np.isfinite(out)
        exact = np.zeros(dx.shape, dtype=bool)
        exact[fin] = _product_is_exact(dx[fin])
    for i in np.flatnonzero(fin & ~exact):
        out[i] = float(FR._rd(Fraction(float(dx[i])) ** 2 + Fraction(float(yy[i]))))
    return out


# ---- the selection with one mistake ---------------------------------------------------------------------------------------
WRONG = ("self_not_excluded", "strict_range", "ties_to_higher_index", "cap_before_range", "radius_of_j_alone",
         "own_post_advance_position", "d2_fma_x", "d2_fma_y", "ties_by_thread_order", "count_of_one_wave", "first_block_only",
         "nan_key_is_zero")


def wrong(kind, c, q=None):
    """the selection of fleet_reference.lists with one mistake (kind None: with none), on q (default: the case's first set)"""
    q = c["q"] if q is None else q
    qp, radius, ns = c["q_post"], c["radius"], c["n_static"]
    B = len(q)
    M = FR.room(ns, c["maxn"])
    with np.errstate(over="ignore"):
        range2 = np.float64(c["rng"]) * np.float64(c["rng"])
    j_all = np.arange(B)
    n_total, rows = np.zeros(B, dtype=np.int32), []
    for y in range(B):
        centre = qp[y] if kind == "own_post_advance_position" else q[y]
        with np.errstate(all="ignore"):
            dx, dy = q[:, 0] - centre[0], q[:, 1] - centre[1]
            if kind == "d2_fma_x":
                d2 = d2_contracted(dx, dy)
            elif kind == "d2_fma_y":
                d2 = d2_contracted(dy, dx)
            else:
                d2 = dx * dx + dy * dy
            if kind == "nan_key_is_zero":
                d2 = np.where(np.isnan(d2), 0.0, d2)
            cand = (d2 < range2) if kind == "strict_range" else (d2 <= range2)
        if kind != "self_not_excluded":
            cand[y] = False
        if kind == "cap_before_range":     # only the first M_y robots (by index) are looked at
            pool = j_all[j_all != y][:M[y]]
            seen = np.zeros(B, dtype=bool)
            seen[pool] = True
            cand &= seen
        if kind == "first_block_only":     # the robots of a thread's second to fourth candidate are never looked at
            cand[KBLOCK:] = False
        idx = np.flatnonzero(cand)
        if kind == "ties_to_higher_index":
            order = np.lexsort((-idx, d2[idx]))
        elif kind == "ties_by_thread_order":   # equal keys in the order the threads hold them
            order = np.lexsort((idx // KBLOCK, idx % KBLOCK, d2[idx]))
        else:
            order = np.lexsort((idx, d2[idx]))
        take = idx[order][:M[y]]
        r = radius[take] if kind == "radius_of_j_alone" else radius[y] + radius[take]
        rows.append(np.stack([q[take, 0], q[take, 1], r], axis=1) if len(take) else np.zeros((0, 3)))
        count = int(np.sum(idx // 64 == 0)) if kind == "count_of_one_wave" else len(idx)   # (one wave's sum for the four totals)
        n_total[y] = int(ns[y]) + min(count, int(M[y]))
    return n_total, rows


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


# ---- the cases of the first fleet change (unchanged) --------------------------------------------------------------------------
def first_cases():
    out = []
    g = np.random.default_rng(20260)
    for i, (B, maxn) in enumerate(((12, 2), (40, 32), (7, 1), (33, 4))):   # random fleets; n_static dealt from {0, 30, 32}
        out.append(_case("random%d" % i, g.uniform(0.0, 5.0, (B, 2)), g.uniform(0.1, 0.6, B), g.choice([0, 30, 32], B), maxn,
                         (1.7, 9.0, 2.5, 1.2)[i]))
    # exact ties: robots 1 and 2 symmetric about robot 0, robot 3 at the same distance on the other axis
    tie = [[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.25, 0.25]]
    for maxn in (1, 2, 32):
        out.append(_case("ties_m%d" % maxn, tie, [0.3, 0.2, 0.25, 0.35, 0.15], 0, maxn, 2.0))
    out.append(_case("ties_room1", tie, 0.3, [31, 0, 30, 32, 0], 3, 2.0))
    # a robot exactly on the range: d2 = 25 = range2; the other one a last place beyond
    out.append(_case("on_range", [[0.0, 0.0], [3.0, 4.0], [0.0, -np.nextafter(5.0, 6.0)]], [0.4, 0.1, 0.2], 0, 2, 5.0))
    # M_y = 0 (a full static list), 1, 2 and 32 (the cap of 32 below the 39 robots in range)
    grid = np.stack(np.meshgrid(np.arange(8) * 0.5, np.arange(5) * 0.5), axis=-1).reshape(-1, 2)
    out.append(_case("grid_m32", grid, np.linspace(0.1, 0.5, len(grid)), 0, 32, 100.0))
    out.append(_case("grid_m0_1_2", grid, 0.2, np.array([32, 31, 30, 0] * 10), 2, 1.0))
    out.append(_case("nobody_in_range", [[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]], 0.3, [0, 30, 32], 2, 0.0))
    out.append(_case("single", [[1.5, -2.0]], 0.3, 0, 4, 10.0))
    return out


# ---- the edges of the device form ---------------------------------------------------------------------------------------------
def sym_pairs():
    """Eight groups of three, 7.3 m apart along the diagonal: an observer at (c, c), c not dyadic, and two robots at offsets
    (a, b) and (b, a) from it -- robot A at (X1, X2) and robot B at (X2, X1), so A's dx is B's dy to the bit and the spec's keys
    are equal: under a cap of 1 the observer takes the lower index.  Contracted, A's key is rd(a^2 + rd(b^2)) in one form and
    rd(b^2 + rd(a^2)) in the other, B's the reverse; the search keeps pairs whose two values differ, placed so that the
    observer's winner flips under fma(dx, dx, dy*dy) for four pairs and under fma(dy, dy, dx*dx) for the other four, A at the
    lower index in one half of each."""
    g = np.random.default_rng(31)
    want = [("x", True), ("x", False), ("y", True), ("y", False)] * 2    # (form that flips the winner, A at the lower index)
    q, pairs, tried, sensitive = [], [], 0, 0
    for k, (form, a_low) in enumerate(want):
        c = 0.1 + 7.3 * k
        while True:
            tried += 1
            x1, x2 = c + g.uniform(0.2, 1.0), c + g.uniform(0.2, 1.0)
            _, ax, ay = d2_forms((x1, x2), (c, c))         # (A's two contracted keys; B's are (ay, ax))
            if ax == ay:
                continue
            sensitive += 1
            # A wins under the x form iff ax < ay; the winner flips where the robot at the higher index wins
            flips = "x" if (ax < ay) != a_low else "y"
            if flips == form:
                break
        A, Bq = [x1, x2], [x2, x1]
        q += [[c, c]] + ([A, Bq] if a_low else [Bq, A])
        pairs.append(dict(observer=3 * k, low=3 * k + 1, high=3 * k + 2, a_low=a_low, flips=form))
    return _case("sym_pairs", q, np.linspace(0.1, 0.4, len(q)), 0, 1, 1.5, info=dict(pairs=pairs, tried=tried, sensitive=sensitive))


def on_range_rounded():
    """range = 0.7 (not dyadic; range2 = rd(range * range)), robot 0 at a centre that is not dyadic, the others at
    (range cos t, range sin t) from it with t searched so that the spec's d2 equals range2 to the bit (in) -- among them, for
    each contracted form, one whose contracted d2 is above range2 --, and one whose d2 is the next double above range2 (out)."""
    g = np.random.default_rng(47)
    rng = 0.7
    range2 = float(FR._rd(Fraction(rng) * Fraction(rng)))
    above = float(np.nextafter(range2, np.inf))
    centre = (0.3, -0.1)
    q, kinds, hits, tried = [centre], [], dict(plain=0, x=0, y=0), 0
    need = dict(plain=4, x=2, y=2, out=1)
    while any(need.values()) and tried < 200000:
        tried += 1
        t = g.uniform(0.0, 2.0 * np.pi)
        p = (centre[0] + rng * np.cos(t), centre[1] + rng * np.sin(t))
        d, fx, fy = d2_forms(p, centre)
        if d == above and need["out"]:
            kind = "out"
        elif d != range2:
            continue
        else:
            kind = "x" if fx > range2 else ("y" if fy > range2 else "plain")
            hits[kind] += 1
            if not need[kind]:
                continue
        need[kind] -= 1
        q.append(p)
        kinds.append(kind)
    return _case("on_range_rounded", q, np.linspace(0.1, 0.3, len(q)), 0, 32, rng,
                 info=dict(kinds=kinds, tried=tried, hits=hits, range2=range2))


def permuted_lattice(B, cols, seed):
    """B cells of a 0.25 m lattice (dyadic: every distance is exact), row-major in `cols` columns, dealt to the robots by a fixed
    seeded permutation: lattice neighbours lie in any stride of the threads' loop and in any wave"""
    cell = np.random.default_rng(seed).permutation(B)
    return np.stack([1.0 + 0.25 * (cell % cols), 0.25 * (cell // cols) - 1.75], axis=1)


def _picks_differ(q, maxn, rng):
    """the robots whose first maxn candidates in (d2, j) order and in (d2, j % 256, j // 256) order are different robots"""
    out = []
    for y in range(len(q)):
        d2 = np.sum((q - q[y]) ** 2, axis=1)
        idx = np.flatnonzero((d2 <= rng * rng) & (np.arange(len(q)) != y))
        a = idx[np.lexsort((idx, d2[idx]))][:maxn]
        b = idx[np.lexsort((idx // KBLOCK, idx % KBLOCK, d2[idx]))][:maxn]
        if sorted(a.tolist()) != sorted(b.tolist()):   # (not the same robots in another order: the cap cuts the tie)
            out.append(y)
    return out


def cross_stride_ties():
    """B = 600 on the permuted lattice, max_neighbours = 2 under a range that holds the four nearest (all at d2 = 0.0625): the
    cap cuts through an exact tie, and for the robots of info['differ'] the tie is between a j with the smaller j % 256 but the
    larger j and the reverse, so the order of the threads and the order of j take different rows"""
    q = permuted_lattice(600, 30, 600)
    return _case("cross_stride_ties", q, 0.1 + 0.001 * np.arange(600), 0, 2, 0.3, info=dict(differ=_picks_differ(q, 2, 0.3)))


def counts_across_waves():
    """B = 1024 on the permuted lattice.  _all: the range holds every robot, n_static dealt from {0, 30, 31, 32} under a cap
    of 32 (M_y = 32, 2, 1, 0; 1023 candidates each).  _cap: max_neighbours = 3 under a range that holds the four nearest, so a
    corner robot has M_y - 1 candidates, an edge robot M_y and an inner robot M_y + 1; info names one of each whose candidates
    lie in different waves both by j // 64 and by (j % 256) // 64, none of them in wave 0."""
    q = permuted_lattice(1024, 32, 1024)
    radius = 0.1 + 0.0005 * np.arange(1024)
    deal = np.random.default_rng(1024).choice([0, 30, 31, 32], 1024)
    named = {}
    for y in range(1024):
        d2 = np.sum((q - q[y]) ** 2, axis=1)
        idx = np.flatnonzero((d2 <= 0.09) & (np.arange(1024) != y))
        key = {2: "below", 3: "at", 4: "above"}[len(idx)]
        if key not in named and len(set(idx // 64)) == len(idx) == len(set((idx % KBLOCK) // 64)) and (idx // 64).min() > 0:
            named[key] = dict(robot=y, candidates=idx.tolist())
    return [_case("counts_across_waves_all", q, radius, deal, 32, 100.0),
            _case("counts_across_waves_cap", q, radius, 0, 3, 0.3, info=dict(named=named))]


BLOCK_SIZES = (2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)


def block_sizes():
    """the permuted lattice (16 columns) cut to B robots, B around every multiple of a wave and of the workgroup up to the
    largest admitted batch: max_neighbours = 4 under a range that holds 12 lattice neighbours, n_static dealt from {0, 30, 32}"""
    out = []
    for B in BLOCK_SIZES:
        deal = np.random.default_rng(B).choice([0, 30, 32], B)
        out.append(_case("block_sizes_B%d" % B, permuted_lattice(B, 16, B), 0.1 + 0.0005 * np.arange(B), deal, 4, 0.5))
    return out


def not_finite():
    """Beside six ordinary robots: a NaN in x, a NaN in y, two robots at x = +inf (inf - inf = NaN between them) and two at
    x = +-1e200 (their dx * dx overflows).  float64 backend only.  info['expect'] states what the spec (numpy) gives:
    _ordinary (range 2): only ordinary robots are candidates, of ordinary robots; the other six have none and are nobody's.
    _huge (range 1e160: range * range = +inf, and d2 = inf <= inf holds): an ordinary robot takes the other five in d2 order,
    then the two at infinity and the two at +-1e200 in index order (all keys +inf); a robot at infinity takes everybody but the
    NaN robots and the other robot at infinity; a robot at +-1e200 everybody but the NaN robots; a NaN robot nobody."""
    g = np.random.default_rng(7)
    inf, nan = np.inf, np.nan
    q = np.concatenate([g.uniform(0.0, 1.2, (6, 2)), [[nan, 0.5], [0.7, nan], [inf, 0.5], [inf, -3.0], [1e200, 0.0], [-1e200, 0.0]]])
    radius = np.linspace(0.1, 0.3, len(q))
    o = list(range(6))
    everybody = lambda y, drop: [j for j in o + [8, 9, 10, 11] if j != y and j not in drop]   # noqa: E731
    huge = {y: everybody(y, ()) for y in o}
    huge.update({6: [], 7: [], 8: everybody(8, (9,)), 9: everybody(9, (8,)), 10: everybody(10, ()), 11: everybody(11, ())})
    ordinary = {y: [j for j in o if j != y] for y in o}
    ordinary.update({y: [] for y in range(6, 12)})
    return [_case("not_finite_ordinary", q, radius, 0, 32, 2.0, q_post=q, finite=False, info=dict(expect=ordinary)),
            _case("not_finite_huge", q, radius, 0, 32, 1e160, q_post=q, finite=False, info=dict(expect=huge))]


def shrinking():
    """Ten robots, one handle, two position sets: first two clusters of five (every robot has 4 neighbours in range), then
    five pairs 2 m apart (every robot has 1).  The rows a robot's list no longer has are where the first set left them."""
    g = np.random.default_rng(10)
    first = np.concatenate([np.array(c) + g.uniform(-0.2, 0.2, (5, 2)) for c in ((1.0, 0.3), (3.0, 0.5))])
    second = np.concatenate([[[0.6 + 2.0 * k, 0.2 + 0.1 * k], [0.9 + 2.0 * k, 0.45 - 0.05 * k]] for k in range(5)])
    return _case("shrinking", first, np.linspace(0.15, 0.3, 10), [0, 3, 0, 0, 28, 0, 0, 1, 0, 0], 4, 0.9, q_next=second)


def new_cases():
    return [sym_pairs(), on_range_rounded(), cross_stride_ties()] + counts_across_waves() + block_sizes() + not_finite() + [shrinking()]


FIRST = first_cases()
NEW = new_cases()
CASES = FIRST + NEW


def cases():
    return list(CASES)

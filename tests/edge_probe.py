"""Inputs that put the disc terms and the grid tap of the batch rollout kernels on their edges, and what the device specs
give there (DESIGN.md sections 10e, 10g, 10h).  Needs no GPU to import.

The disc terms.  The kernels of the four-wave family sum a sample's cost in parts, so a sample's disc penalty is not one fma
chain and differs from form to form.  Two devices take that dependence away.  silent(p) zeroes every weight of the rest of the
cost, so every other addition to a sample's cost is +0.0 (the GPU tests assert it on the term-off run).  And
single_state_discs places the discs -- from the states the device itself stored -- so that at most ONE state of a sample has
g > 0: then every partition and every chain gives fma(w, g_k, 0.0), and a sample without such a state +0.0.  expected_bits
counts the states with g > 0 per sample and gives that cost for counts 0 and 1, by obstacle_cases.spec and
moving_obstacle_reference.spec.

  deep targets      a disc of 1 mm with its centre 0.5 mm from state k_j of sample i_j.  marching(p, v) moves every sample by the
                    same v dt >= 4 cm per step, so the disc cannot hold two states of one sample.
  grazing targets   the centre 0.3 .. 1.5 m from the state, the radius the hypot of the rounded displacement moved by o ulps, o
                    cycling over -2 .. +2: the state is on the edge, and whether it has g > 0 is a matter of the spec's
                    roundings.  The state is a corner of the convex hull of all the instance's states and the disc touches it
                    from outside, so it holds no other state.  A grazing target's sample counts 1 or 0, and both occur.
                    (The issue that asked for these tests also asked that EVERY target count exactly one state, which a
                    grazing target with g == 0 cannot: conditions() asserts one for deep targets, one or none for grazing.)
  moving            velocities of 2 m/s and more, not axis-aligned, the origin o_j = c_j - v_j fl(k_j dt): the disc is at its
                    place at step k_j alone (at k_j +- 1 it is 20 cm away); a grazing one slides along the hull's tangent.
  steps             state 0 is the same for every sample, and so is state 1 of a marching diff-drive instance (the first step
                    is taken at the pose's heading), so a disc there counts for all of them: the instance with one disc has
                    it on state 0, the one with three has all three on state 1 (deep, grazing, grazing: the deep one decides,
                    the others go through the minimum and the padding; steering and full body: on three samples' states 1).
                    The instances with four and 32 discs deal steps() round their deep targets: the first and last state of
                    every block of eight, the last covered state, and two more.
  far discs         the last two discs of an instance with 32 stand at x0 -+ 1e308: a = -2 dx overflows, f is NaN or +inf for
                    every state, and v_min_f64 / fmin drop it.  A minimum that lets a NaN through loses every penalty there.

The grid tap.  grid_probes(g) gives, per axis and per boundary m in {0, 1, n - 1, n}, the two adjacent doubles x across it --
the largest with fx < m and the smallest with fx >= m, fx the reference's own (x - origin) * inv, found by bisection -- and the
origin itself, fx in (-1, 0), fx beyond 2^32 by 2.5 (a wrapping conversion lands in cell 2) and fx about 1e300; the other
coordinate is held mid-cell.  parked(p) keeps a robot where it is, so every covered state of every sample of an instance is
the probe.  probe_maps() are the three maps: a dyadic one and two whose origin and resolution round.

tests/test_edge_probe_cpu.py pins the conditions on the oracle's rollouts; tests/test_gpu_batch_edges.py asserts them on the
device's states.
"""
import math

import numpy as np

import batch_support as BS
import grid_reference as GR
import moving_obstacle_reference as MR
import obstacle_cases as OC

W_EDGE = 7.3          # (not dyadic: w g rounds)
V_MARCH = 0.8         # m/s: 8 cm per step at dt = 0.1
DEEP_R, DEEP_OFF = 1.0e-3, 0.5e-3
GRAZE_RHO = (0.3, 0.6, 1.0, 1.5)
FAR = 1.0e308
EPS = 1.0e-9          # m^2: an approximate power farther than this from 0 has the sign the spec's s has (the error is ~1e-14)
MARGIN = 1.0e-6       # m^2: the states of a target that must not count stay this far outside every disc
WRONG_STATIC = ("gpos", "nanmin")
WRONG_MOVING = ("early", "late", "local", "gpos", "nanmin")


# ---- parameters -------------------------------------------------------------------------------------------------------------
def silent(p):
    """p with every weight of the rest of the cost zero: the term-off cost of every sample is +0.0"""
    return p.with_(path_weight=0.0, v_weight=0.0, zmp_weight=0.0, roll_v_weight=0.0, back_weight=0.0, yaw_weight=0.0)


def marching(p, v):
    """p with the speed bounds u_min[0] = u_max[0] = v: every sample advances by v dt per step, the noise still spreads the
    headings"""
    return p.with_(u_min=(float(v),) + tuple(p.u_min[1:]), u_max=(float(v),) + tuple(p.u_max[1:]))


def parked(p):
    """marching(p, 0.0): every state of every sample is the pose (the GPU tests assert it on the stored states)"""
    return marching(p, 0.0)


def march_params(p, B):
    """B silent parameter sets, instance b marching at V_MARCH (1 + 0.1 (b % 3))"""
    return [marching(silent(p), V_MARCH * (1.0 + 0.1 * (b % 3))) for b in range(B)]


def disc_counts(B):
    """the discs per instance, dealt round: obstacle_cases.NS, or (3, 32) for a batch of two"""
    return OC.NS if B >= len(OC.NS) else (3, 32)


def lead_of(B, n, alt):
    """the shared state the discs of an instance with one or three discs stand on: 0 and 1 -- a batch of two has no instance
    with one disc, and its instance with three takes state 0 or, with `alt`, state 1"""
    if n == 1:
        return 0
    return 1 if (B >= len(OC.NS) or alt) else 0


def is_parked(P, x0):
    """every state of P [K][T][2] equals the pose in every bit"""
    P = np.ascontiguousarray(P, dtype=np.float64)
    want = np.broadcast_to(np.asarray(x0[:2], dtype=np.float64), P.shape)
    return P.tobytes() == np.ascontiguousarray(want).tobytes()


# ---- discs ------------------------------------------------------------------------------------------------------------------
def steps(T):
    """the steps dealt round the targets of an instance with four or 32 discs: the first and last state of every block of eight
    from state 2 on, the last covered state, and states 3 and T // 2 (at state 2 the samples lie within millimetres of each
    other: a disc of 1 mm there holds a tenth of them)"""
    out = {3, T // 2, T - 1}
    for b in range((T + 7) // 8):
        out |= {8 * b, 8 * b + 7}
    return sorted(k for k in out if 2 <= k < T)


def ulps(x, o):
    """x moved by o units in the last place"""
    for _ in range(abs(int(o))):
        x = float(np.nextafter(x, math.inf if o > 0 else -math.inf))
    return float(x)


def velocity(j):
    """disc j's velocity: 2 m/s and more, at least 0.3 rad from either axis"""
    ang = 0.5 + 0.9 * j
    while min(abs(math.sin(ang)), abs(math.cos(ang))) < 0.3:
        ang += 0.35
    mag = 2.0 + 0.25 * (j % 5)
    return np.array([mag * math.cos(ang), mag * math.sin(ang)])


def is_shared(P, k):
    """state k of P [K][T][2] is the same for every sample: state 0 always, and state 1 of a marching diff-drive instance,
    whose first step is taken at the pose's heading (steering and full body turn the first step by a sampled angle)"""
    return bool(np.all(P[:, k] == P[0, k]))


def _near(discs):
    d = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    return np.all(np.abs(d[:, :2]) < 1.0e100, axis=1)


def disc_power(P, ks, dt, disc, vel=None):
    """|P_k - o - v k dt|^2 - r^2 of one disc for states P [K][T][2] at the steps ks [T], in plain float64: approximate"""
    tau = np.asarray(ks, dtype=np.float64) * float(dt)
    vx, vy = (0.0, 0.0) if vel is None else (float(vel[0]), float(vel[1]))
    ex = P[..., 0] - (disc[0] + vx * tau)
    ey = P[..., 1] - (disc[1] + vy * tau)
    return ex * ex + ey * ey - disc[2] * disc[2]


def hull(points):
    """the convex hull of points [N][2], counter-clockwise: a list of (index into points, the two unit outward normals of the
    edges that meet there).  (Andrew's monotone chain on the distinct points; collinear points are left out.)"""
    pts, first = np.unique(np.asarray(points, dtype=np.float64), axis=0, return_index=True)   # (sorted by x, then y)
    if len(pts) < 3:
        return []

    def chain(order):
        out = []
        for t in order:
            while len(out) >= 2:
                a, b = pts[out[-2]], pts[out[-1]]
                if (b[0] - a[0]) * (pts[t][1] - a[1]) - (b[1] - a[1]) * (pts[t][0] - a[0]) > 0.0:
                    break
                out.pop()
            out.append(t)
        return out

    lower, upper = chain(range(len(pts))), chain(range(len(pts) - 1, -1, -1))
    ring_ = lower[:-1] + upper[:-1]
    out = []
    for a, b, c in zip(ring_[-1:] + ring_[:-1], ring_, ring_[1:] + ring_[:1]):
        e1, e2 = pts[b] - pts[a], pts[c] - pts[b]
        n1, n2 = np.array([e1[1], -e1[0]]) / np.hypot(*e1), np.array([e2[1], -e2[0]]) / np.hypot(*e2)
        out.append((int(first[b]), n1, n2))
    return out


def _off_axis(t):
    return min(abs(t[0]), abs(t[1])) / float(np.hypot(*t)) > math.sin(0.3)


def _graze(st, nrm, rho, o_ulps, k, dt, moving, j):
    """the disc that touches the state st from the side the unit normal nrm points to: the centre rho along nrm (rounded), the
    radius the hypot of the rounded displacement moved by o_ulps; with `moving` it slides along the tangent -- it stays on
    its side of the tangent line at every time -- at velocity(j)'s speed, and is at its place at fl(k dt)"""
    c = st + rho * nrm
    dx, dy = float(c[0] - st[0]), float(c[1] - st[1])
    r = ulps(float(np.hypot(dx, dy)), o_ulps)
    if not moving:
        return np.array([c[0], c[1], r]), None
    tan = np.array([-nrm[1], nrm[0]]) * (1.0 if j % 4 < 2 else -1.0)
    v = float(np.hypot(*velocity(j))) * tan
    o = c - v * (float(k) * float(dt))
    return np.array([o[0], o[1], r]), v


def _deep(st, k, dt, moving, j, t):
    ang = 2.399963 * j + 1.5707963 * t
    c = st + DEEP_OFF * np.array([math.cos(ang), math.sin(ang)])
    v = velocity(j) if moving else None
    o = c if v is None else c - v * (float(k) * float(dt))
    return np.array([o[0], o[1], DEEP_R]), v


def step_disc(st, k, dt, j):
    """(disc [3], velocity [2]): the deep moving disc that is on the state st at step k alone"""
    return _deep(np.asarray(st, dtype=np.float64), k, dt, True, j, 0)


def single_state_discs(P, x0, dt, n, moving, lead=None):
    """n discs on the stored states P [K][T][2] of one instance (module docstring) -> (discs [n][3], velocities [n][2] or None,
    targets: a list of (sample i_j, step k_j, "deep" | "grazing", disc j)).

    n = 1: one deep disc on state `lead` (0).  n = 3, where every sample shares state `lead` (1): a deep and two grazing discs
    on it, the grazing ones across the way of the samples, 0.3 m to either side, tilted so that they hold another state of the
    fewest samples; the target is the first sample of which they hold none.  n = 4, 32 (and n = 3 where state `lead` differs
    from sample to sample): deep (even j) and grazing (odd j) on different samples.  The deep ones at steps(T) dealt round, on
    the samples in order.  The grazing ones on corners of the convex hull of ALL the states, from outside, along a normal of
    the hull there: such a disc, of any radius, holds no other state; moving, it slides along the hull's tangent and never
    does.  The hull's corners are states of the fan's front and flanks; corners on a shared state are left out; when the
    corners run out the hull of the samples that had none is taken, up to eight times, and then a deep disc takes the grazing
    one's place.  A disc is taken only if it leaves every state of every other target outside by MARGIN, and the other states
    of its own.  n = 32: the last two discs are the far ones."""
    P = np.asarray(P, dtype=np.float64)
    K, T = P.shape[:2]
    ks = np.arange(T)
    if n == 0:
        return np.zeros((0, 3)), (np.zeros((0, 2)) if moving else None), []
    n_far = 2 if n >= 32 else 0
    m = n - n_far
    found = {}     # j -> (disc, velocity, sample, step, kind)
    s_all = np.full((K, T), np.inf)
    taken = []

    def fits(q, i, k):
        if np.any(np.delete(q[i], k) <= MARGIN):
            return False
        return not (taken and np.any(q[taken] <= MARGIN))

    def take(j, disc, v, q, i, k, kind):
        nonlocal s_all
        s_all = np.minimum(s_all, q)
        taken.append(i)
        found[j] = (disc, v, i, k, kind)

    k = (0 if n == 1 else 1) if lead is None else int(lead)
    if n in (1, 3) and is_shared(P, k):
        lo, hi = max(k - 1, 0), min(k + 1, T - 1)
        way = (P[:, hi] - P[:, lo]).mean(axis=0)
        nrm = np.array([-way[1], way[0]]) / np.hypot(*way)
        fwd = way / np.hypot(*way)
        chosen, bad = [], np.zeros(K, dtype=bool)
        for j in range(n):   # per disc: of the tilts of its side, the one that holds another state of the fewest samples
            if j == 0:
                cands = [_deep(P[0, k], k, dt, moving, 0, 0)]
            else:
                side = nrm if j == 1 else -nrm
                cands = [_graze(P[0, k], (side + t * fwd) / np.hypot(*(side + t * fwd)), GRAZE_RHO[0], (-1, 1)[j - 1], k, dt, moving, j)
                         for t in (0.0, -0.1, 0.1, -0.2, 0.2)]
            qs = [disc_power(P, ks, dt, disc, v) for disc, v in cands]
            held = [np.any(np.delete(q, k, axis=-1) <= MARGIN, axis=1) for q in qs]
            t = int(np.argmin([h.sum() for h in held]))
            chosen.append((cands[t], qs[t]))
            bad |= held[t]
        assert not bad.all(), "every sample has another state in a disc on the shared state %d" % k
        i = int(np.argmin(bad))   # the target: the first sample of which no other state is held
        for j, ((disc, v), q) in enumerate(chosen):
            take(j, disc, v, q, i, k, "deep" if j == 0 else "grazing")
    else:
        st = [k] if n in (1, 3) else steps(T)   # (steering, full body: state 1 differs from sample to sample)
        nxt = 0

        def deep(j):
            nonlocal nxt
            k = st[(j // 2) % len(st)]
            while j not in found:
                i, nxt = nxt, nxt + 1
                assert i < K, "no sample left for deep disc %d" % j
                if i in taken or np.any(s_all[i] <= MARGIN):
                    continue   # a target already, or an earlier disc holds a state of this sample
                for t in range(4):
                    disc, v = _deep(P[i, k], k, dt, moving, j, t)
                    q = disc_power(P, ks, dt, disc, v)
                    if fits(q, i, k):
                        take(j, disc, v, q, i, k, "deep")
                        break

        for j in range(0, m, 2):
            deep(j)
        js = list(range(1, m, 2))
        left = np.arange(K)   # the samples whose states the hull is taken of: all, then without those that had a corner (a disc
        for layer in range(8):   # on an inner hull may hold states of the samples peeled off: `fits` keeps the targets out)
            if not js or len(left) == 0:
                break
            corners = hull(P[left].reshape(-1, 2))
            seen = set()
            for flat, n1, n2 in corners:   # grazing
                i, k = divmod(flat, T)
                i = int(left[i])
                seen.add(i)
                if not js or is_shared(P, k) or i in taken or np.any(s_all[i] <= MARGIN):
                    continue
                j = js[0]
                for mix in (0.5, 0.25, 0.75):
                    nrm = mix * n1 + (1.0 - mix) * n2
                    nrm = nrm / np.hypot(*nrm)
                    if moving and not _off_axis(nrm):   # (the tangent is off the axes where the normal is)
                        continue
                    disc, v = _graze(P[i, k], nrm, GRAZE_RHO[(j // 2) % len(GRAZE_RHO)], (j // 2) % 5 - 2, k, dt, moving, j)
                    q = disc_power(P, ks, dt, disc, v)
                    if fits(q, i, k):
                        take(j, disc, v, q, i, k, "grazing")
                        js.pop(0)
                        break
            left = np.array([i for i in left if i not in seen], dtype=np.int64)
        for j in js:   # no corner left (few samples, or every tangent near an axis): a deep disc in the grazing one's place
            deep(j)
    discs = [found[j][0] for j in range(m)]
    vels = [found[j][1] if moving else np.zeros(2) for j in range(m)]
    targets = [(found[j][2], found[j][3], found[j][4], j) for j in range(m)]
    for sgn in (1.0, -1.0)[:n_far]:
        discs.append(np.array([x0[0] + sgn * FAR, x0[1] + 1.0, 1.0]))
        vels.append(np.zeros(2))
    return np.array(discs).reshape(-1, 3), (np.array(vels).reshape(-1, 2) if moving else None), targets


def near_discs(discs, vels):
    """the discs without the far ones (which never count), for the references that work in real arithmetic"""
    keep = _near(discs)
    d = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[keep]
    return d, (None if vels is None else np.asarray(vels, dtype=np.float64).reshape(-1, 2)[keep])


# ---- what the spec gives ----------------------------------------------------------------------------------------------------
def spec_of(P1, ks1, x0, dt, discs, vels, w, wrong=None):
    """(s, g, cost) of the states P1 [T][2] of one sample by the spec of the term the velocities choose"""
    if vels is None:
        return OC.spec(P1, x0, discs, w, wrong, parts=True)
    return MR.spec(P1, ks1, x0, dt, discs, vels, w, wrong, parts=True)


def expected_bits(P, ks, x0, dt, discs, vels, w, wrong=None, samples=None):
    """(count [K], cost [K]) for states P [K][T][2] at the steps ks [T]: the number of states with g > 0 by the spec, and the cost
    the device must have in every bit where that number is 0 (+0.0) or 1 (fma(w, g_k, 0.0)); NaN where it is larger.  vels
    None: the static term.

    Without `wrong`: the sign of s is taken from a float64 evaluation of the power wherever that is farther than EPS from 0
    (its error is ~1e-14 m^2), and from the spec elsewhere; the one counted state's g is the spec's, evaluated over the discs
    whose power there lies within EPS of the smallest -- the others cannot be the minimum, and the minimum over a list is the
    minimum over any part of it that holds the smallest.  Far discs never count (f is NaN or +inf: dropped by the minimum).
    With `wrong`, or `samples` (indices; the other samples get count -1): the whole spec over the whole list for every
    state of those samples, and the cost is the chain's whatever the count."""
    P = np.asarray(P, dtype=np.float64)
    K, T = P.shape[:2]
    ks = np.asarray(ks, dtype=np.int64)
    discs = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    n = discs.shape[0]
    if wrong is not None or samples is not None:
        count, cost = np.full(K, -1, dtype=np.int64), np.full(K, np.nan)
        for i in (range(K) if samples is None else samples):
            _, g, c = spec_of(P[i], ks, x0, dt, discs, vels, w, wrong)
            count[i], cost[i] = int(np.count_nonzero(g > 0)), c
        return count, cost
    count, cost = np.zeros(K, dtype=np.int64), np.zeros(K)
    if n == 0:
        return count, cost
    near = np.flatnonzero(_near(discs))
    v_of = (lambda j: None) if vels is None else (lambda j: np.asarray(vels, dtype=np.float64).reshape(-1, 2)[j])
    s, s2, arg = np.full((K, T), np.inf), np.full((K, T), np.inf), np.zeros((K, T), dtype=np.int64)
    for j in near:   # the smallest power, the disc it belongs to, and the second smallest
        q = disc_power(P, ks, dt, discs[j], v_of(j))
        first = q < s
        s2 = np.where(first, s, np.minimum(s2, q))
        arg = np.where(first, j, arg)
        s = np.where(first, q, s)
    hit = s < -EPS
    cache = {}

    def exact(i, k):
        key = (P[i, k].tobytes(), int(ks[k]))
        if key not in cache:
            if s2[i, k] > s[i, k] + EPS:
                part = arg[i, k:k + 1]
            else:
                q = np.array([disc_power(P[i, k], ks[k:k + 1], dt, discs[j], v_of(j))[0] for j in near])
                part = near[q <= q.min() + EPS]
            sub_v = None if vels is None else np.asarray(vels, dtype=np.float64).reshape(-1, 2)[part]
            _, g, c = spec_of(P[i, k:k + 1], ks[k:k + 1], x0, dt, discs[part], sub_v, w)
            cache[key] = (float(g[0]), c)
        return cache[key]

    for i, k in zip(*np.nonzero(np.abs(s) <= EPS)):   # on an edge: the spec decides
        hit[i, k] = exact(i, k)[0] > 0
    count = hit.sum(axis=1)
    for i in np.flatnonzero(count == 1):
        cost[i] = exact(i, int(np.argmax(hit[i])))[1]
    cost[count >= 2] = np.nan
    return count, cost


def conditions(what, count, targets, n):
    """the conditions on one instance's inputs, asserted: a deep target's sample counts exactly one state; a grazing target's
    one or none (in an instance whose discs share a state, where the deep disc decides: one); no more than a quarter of the
    samples count two or more.  -> (grazing targets with g > 0, with g == 0) of an instance whose discs stand on different
    samples"""
    shared = len({i for i, _, _, _ in targets}) == 1   # (else: as many samples as targets)
    assert shared or len({i for i, _, _, _ in targets}) == len(targets), what
    pos = zero = 0
    for i, k, kind, j in targets:
        if kind == "deep" or shared:
            assert count[i] == 1, (what, "target", i, k, kind, int(count[i]))
        else:
            assert count[i] in (0, 1), (what, "target", i, k, kind, int(count[i]))
            pos, zero = pos + int(count[i] == 1), zero + int(count[i] == 0)
    if n:
        assert np.mean(count >= 2) <= 0.25, (what, float(np.mean(count >= 2)))
    return pos, zero


def bits_equal(a, b):
    return np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)


# ---- grid probes ------------------------------------------------------------------------------------------------------------
def probe_maps():
    """a dyadic map (every fx is exact) and two whose origin and resolution round; as grid_reference.map_ahead makes them: nx !=
    ny, neither a power of two, every cell a distinct small integer, `outside` a value no cell has"""
    def cells(nx, ny):
        return (1.0 + np.arange(nx * ny, dtype=np.float64)).reshape(ny, nx).astype(np.float32)
    return [GR.Grid(cells(13, 11), (-2.0, -2.0), 0.125, -2.5), GR.Grid(cells(11, 14), (0.1, -0.7), 0.05, -3.5),
            GR.Grid(cells(14, 9), (1234567.3, -7654321.7), 0.03, -4.5)]


def _f(x, origin, inv):
    return float((np.float64(x) - np.float64(origin)) * np.float64(inv))


def straddle(origin, inv, res, m):
    """the adjacent doubles (lo, hi) with f(lo) < m <= f(hi), f(x) = (x - origin) * inv as the reference rounds it"""
    lo, hi = origin + (m - 1) * res, origin + (m + 1) * res
    assert _f(lo, origin, inv) < m <= _f(hi, origin, inv)
    while float(np.nextafter(lo, math.inf)) != hi:
        mid = lo + (hi - lo) / 2
        if mid <= lo or mid >= hi:
            mid = float(np.nextafter(lo, math.inf))
        if _f(mid, origin, inv) < m:
            lo = mid
        else:
            hi = mid
    return lo, hi


def grid_probes(g):
    """(states [N][2], names [N], pairs: a list of (index of lo, index of hi, axis, m)) for the map g (module docstring)"""
    mid = (g.ox + (g.nx // 2 + 0.5) * g.resolution, g.oy + (g.ny // 2 + 0.5) * g.resolution)
    states, names, pairs = [], [], []

    def add(axis, v, name):
        states.append((v, mid[1]) if axis == 0 else (mid[0], v))
        names.append("%s %s" % ("xy"[axis], name))
        return len(states) - 1

    for axis, (origin, n) in enumerate(((g.ox, g.nx), (g.oy, g.ny))):
        for m in (0, 1, n - 1, n):
            lo, hi = straddle(origin, g.inv, g.resolution, m)
            pairs.append((add(axis, lo, "below %d" % m), add(axis, hi, "at %d" % m), axis, m))
        add(axis, origin, "origin")
        add(axis, float(np.nextafter(origin, -math.inf)), "tiny negative")
        add(axis, origin - 0.5 * g.resolution, "in (-1, 0)")
        add(axis, origin + (2.0 ** 32 + 2.5) * g.resolution, "2^32 + 2.5")
        add(axis, 1.0e300, "1e300")
    return np.array(states, dtype=np.float64), names, pairs


def probe_inputs(p, states, extra_heading=None):
    """the inputs of a batch with one parked instance per probe state -- the pose at the state with heading 0.3, a window
    running off along x, warm starts of zeros; extra_heading: one more instance, at the first state, with that heading"""
    states = np.asarray(states, dtype=np.float64)
    if extra_heading is not None:
        states = np.concatenate([states, states[:1]])
    B = len(states)
    x0 = np.zeros((B, 5 if p.model == "full_body" else 3))
    x0[:, :2] = states
    x0[:, 2] = 0.3
    if extra_heading is not None:
        x0[-1, 2] = extra_heading
    xr = x0[:, :1] + 0.08 * np.arange(p.horizon)[None, :]
    yr = np.repeat(x0[:, 1:2], p.horizon, axis=1)
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)
    return x0, np.full(B, p.dt), xr, yr, np.zeros(B), seeds, np.zeros((B, p.horizon - 1, p.udim))

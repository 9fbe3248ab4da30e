"""Reference of the batch handles' moving-disc term and the rounding bound of its device spec (test helper, CPU only; the
pattern of obstacle_reference.py, whose static term this one equals exactly when every velocity is zero).

The term (include/ccv_mppi.h, ccv_mppi_batch_set_obstacle_velocities).  State k of a sample -- k
dynamics steps after the pose, state 0 the pose itself -- at the fp64 position P_k, discs (ox_j, oy_j, r_j) with velocities
(vx_j, vy_j), j < n, the rollout's fp64 dt and a weight w >= 0:

    tau_k      = k dt                                            (the real product)
    power_k    = min_j ( |P_k - o_j - v_j tau_k|^2 - r_j^2 )     (+inf for n = 0)
    penalty_k  = w * max(-power_k, 0)                            (0 for a NaN position)

as real-number functions of the fp64 inputs.  Arithmetic: numpy.longdouble where it has a 64-bit mantissa, the displacement
formed as (X - ox) - vx tau -- k dt is exact there for k < 2^11, and with v = 0 the expression is obstacle_reference.power's,
operation for operation; elsewhere exact rationals (`backend="exact"` forces them; the pinning test holds the two together).

The device spec (u = 2^-53; x0 the pose the kernel holds, fl() one fp64 rounding, every fma written out):

    staging   dx, dy, a = -2 dx, b = -2 dy, c as in obstacle_reference;  va = -2 vx, vb = -2 vy (exact);
              c1 = 2 fma(dx, vx, fl(dy vy));  c2 = fma(vx, vx, fl(vy vy));  the padding has a = b = va = vb = c1 = c2 = 0, c = +inf
    state k   tau = fl(double(k) dt),  k the GLOBAL step index of the state
              at = fma(va, tau, a);  bt = fma(vb, tau, b);  ct = fma(fma(c2, tau, c1), tau, c)
              f_j = fma(at, p_x, fma(bt, p_y, ct));  m = min_j f_j;  s = fl(m + fma(p_x, p_x, fl(p_y p_y)))
              g = max(-s, 0) (NaN -> 0);  cost = fma(w, g, cost)

The bound of s, term by term, against power_k = |p* - d* - v tau*|^2 - r^2 (p* = P - x0, d* = o - x0, tau* = k dt unrounded).
Second-order terms are dropped and counts rounded up.  Magnitudes: Ax = |a| + |va| tau, By = |b| + |vb| tau,
C1 = 2 (|dx vx| + |dy vy|), D = |v|^2 tau^2 + C1 tau + |d|^2 + r^2 (>= |ct|), |p|^2 = p_x^2 + p_y^2.

    tau   one rounding: |tau - tau*| <= u tau  (double(k) is exact)
    at    a carries dx's rounding (u |a|); va tau carries tau's (u |va| tau); the fma u |at| <= u Ax          <= 2 u Ax;  bt alike
    c2    fl(vy vy) and the fma                                                                              <= 2 u |v|^2
    c1    fl(dy vy): u |dy vy|;  the fma: u C1 / 2;  dx, dy's roundings: u C1 / 2;  times 2                   <= 3 u C1
    inner fma(c2, tau, c1): c2's error times tau (2 u |v|^2 tau), tau's (u |v|^2 tau), c1's (3 u C1), its own
          rounding u (|v|^2 tau + C1)                                                                        <= 4 u (|v|^2 tau + C1)
    ct    the inner error times tau: 4 u (|v|^2 tau^2 + C1 tau);  tau's own: u (|v|^2 tau^2 + C1 tau);  c's error
          5 u (|d|^2 + r^2) (obstacle_reference);  the fma: u D                                              <= 6 u D
    f_j   at's error and p_x's rounding: 3 u Ax |p_x|;  bt, p_y: 3 u By |p_y|;  the inner fma: u (By |p_y| + D);  the outer:
          u (Ax |p_x| + By |p_y| + D);  ct's error                                      <= u [5 (Ax |p_x| + By |p_y|) + 8 D]
    |p|^2 4 u |p|^2 (obstacle_reference);   s: the sum, u (Ax |p_x| + By |p_y| + D + |p|^2)
    min   |min_j f_j - min_j f*_j| <= max_j |f_j - f*_j|

    |s - power_k| <= 9 u S,   S = max_j ( Ax_j |p_x| + By_j |p_y| + D_j ) + |p|^2

With every velocity zero S is obstacle_reference's S.  S_ULPS = 10 is the 9 above and one for the dropped terms.  The new
magnitudes are |v| tau and the rounding of tau itself: at the reference's operating point (|v| tau <= 2 m at step 14) they
leave S at the size of the static term's; at step 127 with dt = 0.1 and |v| = 1.5 m/s, |v| tau = 19 m enters S squared.

The reference's own error (longdouble): the two displacements carry three roundings each (X - ox, vx tau, their difference),
their squares, the sum and r^2 one each: below 16 * 2^-64 of (|p| + |d| + |v| tau)^2 + r^2 <= 3 S; REF_ULPS = 64 charges 2^-58 S.

    penalty of one state     w (S_ULPS u + REF_ULPS 2^-64) S
    a sample's T states and the difference of two runs: obstacle_reference.sample_penalty's and bound_difference's reasoning,
    unchanged (the term adds the same T fma's to the running cost).

They are derived, not tuned.  test_moving_obstacle_reference.py shows the numpy restatement of the spec (spec, below) inside
them and seven wrong versions outside; tests/edge_probe.py holds the device against the same restatement bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

import obstacle_reference as OR

LD = np.longdouble
U = OR.U
HAVE_LD = OR.HAVE_LD
S_ULPS = 10
REF_ULPS = 64
CHUNK = 1 << 12   # samples per piece (x T states x n discs)
bound_difference = OR.bound_difference


def _vel(vel, n):
    v = np.zeros((n, 2)) if vel is None else np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    assert v.shape[0] == n, "one velocity per disc"
    return v


def _steps(P, k):
    k = np.asarray(k, dtype=np.int64).reshape(-1)
    assert P.shape[-2] == k.shape[0], "one step index per state"
    return k


def power(P, k, dt, discs, vel, backend=None):
    """min_j |P_k - o_j - v_j k dt|^2 - r_j^2 for fp64 positions P [..., T, 2] at the steps k [T]: longdouble [..., T] (+inf
    without discs, NaN for a NaN position)."""
    P = np.asarray(P, dtype=np.float64)
    d = OR._discs(discs)
    v = _vel(vel, d.shape[0])
    k = _steps(P, k)
    shape = P.shape[:-1]
    T = k.shape[0]
    if d.shape[0] == 0:
        out = np.full(shape, np.inf, dtype=LD)
        out[np.isnan(P).any(axis=-1)] = np.nan
        return out
    flat = P.reshape(-1, T, 2)
    out = np.empty(flat.shape[:2], dtype=LD)
    if backend == "exact" or (backend is None and not HAVE_LD):
        fdt = Fraction(float(dt))
        fd = [(Fraction(float(ox)), Fraction(float(oy)), Fraction(float(r))) for ox, oy, r in d]
        fv = [(Fraction(float(vx)), Fraction(float(vy))) for vx, vy in v]
        for i in range(flat.shape[0]):
            for t in range(T):
                x, y = flat[i, t]
                if not (np.isfinite(x) and np.isfinite(y)):
                    out[i, t] = np.nan
                    continue
                fx, fy, tau = Fraction(float(x)), Fraction(float(y)), int(k[t]) * fdt
                q = min((fx - ox - vx * tau) ** 2 + (fy - oy - vy * tau) ** 2 - r ** 2 for (ox, oy, r), (vx, vy) in zip(fd, fv))
                hi = float(q)
                out[i, t] = LD(hi) + LD(float(q - Fraction(hi)))
        return out.reshape(shape)
    assert int(k.max(initial=0)) < 2048   # (k dt exact in longdouble)
    ox, oy, r = d[:, 0].astype(LD), d[:, 1].astype(LD), d[:, 2].astype(LD)
    tau = k.astype(LD) * LD(float(dt))                                  # [T], exact
    sx, sy = v[:, 0].astype(LD) * tau[:, None], v[:, 1].astype(LD) * tau[:, None]   # [T][n]
    for i in range(0, flat.shape[0], CHUNK):
        X, Y = flat[i:i + CHUNK, :, 0].astype(LD)[..., None], flat[i:i + CHUNK, :, 1].astype(LD)[..., None]
        with np.errstate(invalid="ignore"):
            ex, ey = (X - ox) - sx, (Y - oy) - sy
            q = ex * ex + ey * ey - r * r
            out[i:i + CHUNK] = np.min(q, axis=-1)
    return out.reshape(shape)


def penalty(P, k, dt, discs, vel, w, backend=None):
    """w * max(-power, 0) per state, longdouble [..., T]; 0 for a NaN position and without discs."""
    s = power(P, k, dt, discs, vel, backend)
    with np.errstate(invalid="ignore"):
        g = np.where(s < 0, -s, LD(0))
    return LD(w) * g


def scale(P, x0, k, dt, discs, vel):
    """S of the module docstring per state, fp64 [..., T]; 0 without discs, NaN for a NaN position."""
    P = np.asarray(P, dtype=np.float64)
    d = OR._discs(discs)
    v = _vel(vel, d.shape[0])
    k = _steps(P, k)
    T = k.shape[0]
    px, py = P[..., 0] - x0[0], P[..., 1] - x0[1]
    p2 = px * px + py * py
    if d.shape[0] == 0:
        return np.zeros(P.shape[:-1]) + 0.0 * p2
    tau = np.abs(k.astype(np.float64) * float(dt))[:, None]            # [T][1]
    dx, dy, r = d[:, 0] - x0[0], d[:, 1] - x0[1], d[:, 2]
    vx, vy = v[:, 0], v[:, 1]
    Ax = np.abs(2.0 * dx) + np.abs(2.0 * vx) * tau                     # [T][n]
    By = np.abs(2.0 * dy) + np.abs(2.0 * vy) * tau
    D0 = dx * dx + dy * dy + r * r                                     # (the static term's part first, in its order: v = 0 gives
    Dv = (vx * vx + vy * vy) * tau * tau + 2.0 * (np.abs(dx * vx) + np.abs(dy * vy)) * tau   # obstacle_reference.scale exactly)
    fx, fy = np.abs(px).reshape(-1, T), np.abs(py).reshape(-1, T)
    out = np.empty(fx.shape)
    for i in range(0, fx.shape[0], CHUNK):
        per = D0 + Ax * fx[i:i + CHUNK, :, None] + By * fy[i:i + CHUNK, :, None] + Dv
        out[i:i + CHUNK] = np.max(per, axis=-1)
    return out.reshape(px.shape) + p2


def bound_s(P, x0, k, dt, discs, vel):
    """|device s - power| per state (states with discs and a finite position)."""
    return (S_ULPS * U + REF_ULPS * 2.0 ** -64) * scale(P, x0, k, dt, discs, vel) * (1.0 + 2.0 ** -20)


def bound_penalty(P, x0, k, dt, discs, vel, w):
    """|w * device g - penalty| per state; 0 for a NaN position (the device's 0 is exact)."""
    b = float(w) * bound_s(P, x0, k, dt, discs, vel)
    return np.where(np.isnan(b), 0.0, b)


KTU = 8   # the kernels' block of states


def spec(P, ks, x0, dt, discs, vel, w, wrong=None, parts=False):
    """The device spec for states P [T][2] of one sample at the global steps ks [T]: (s [T], cost after the T fma's from 0.0);
    with `parts` (s [T], g [T], cost).  wrong: one mistake, by name -- "sign", "xonly", "cross1", "notau2", "nodt", "late" (tau of
    k + 1), "early" (tau of k - 1), "local" (k inside the block of eight in place of the global step), "gpos" (g = max(s, 0)),
    "nanmin" (a minimum that lets a NaN f through)."""
    fma, fmin = OR.fma, OR.fmin
    discs = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    n = discs.shape[0]
    rows = []
    for (ox, oy, r), (vx, vy) in zip(discs, vel):
        if wrong == "sign":
            vx, vy = -vx, -vy
        if wrong == "xonly":
            vy = 0.0
        dx, dy = float(ox - x0[0]), float(oy - x0[1])
        c = fma(dx, dx, dy * dy) - r * r
        c1 = (1.0 if wrong == "cross1" else 2.0) * fma(dx, vx, dy * vy)
        c2 = 0.0 if wrong == "notau2" else fma(vx, vx, vy * vy)
        rows.append((-2.0 * dx, -2.0 * dy, c, -2.0 * vx, -2.0 * vy, c1, c2))
    s_out, g_out, cost = [], [], 0.0
    for (X, Y), k in zip(np.asarray(P, dtype=np.float64), ks):
        k = int(k)
        if wrong == "late":
            k = k + 1
        if wrong == "early":
            k = k - 1
        if wrong == "local":
            k = k % KTU
        tau = float(k) if wrong == "nodt" else float(k) * float(dt)
        px, py = float(X - x0[0]), float(Y - x0[1])
        p2 = fma(px, px, py * py)
        if n == 0:
            s_out.append(math.inf if px == px and py == py else math.nan)
            g_out.append(0.0)
            continue
        m = math.inf
        for a, b, c, va, vb, c1, c2 in rows:
            at, bt = fma(va, tau, a), fma(vb, tau, b)
            ct = fma(fma(c2, tau, c1), tau, c)
            f = fma(at, px, fma(bt, py, ct))
            m = OR.nanmin(m, f) if wrong == "nanmin" else fmin(m, f)
        s = m + p2
        s_out.append(s)
        if wrong == "gpos":
            g = max(s, 0.0) if s == s else 0.0
        else:
            g = max(-s, 0.0) if s == s else 0.0   # v_max_f64(-s, 0): NaN -> 0
        g_out.append(g)
        cost = fma(w, g, cost)
    if parts:
        return np.array(s_out), np.array(g_out), cost
    return np.array(s_out), cost


def sample_penalty(P, x0, k, dt, discs, vel, w, backend=None):
    """P [K][T][2] at the steps k [T] -> (sum_t penalty [K] as longdouble, its bound [K]) for the fma chain onto a cost that
    starts at 0."""
    pen = penalty(P, k, dt, discs, vel, w, backend)
    tot = pen.sum(axis=-1)
    T = pen.shape[-1]
    bnd = bound_penalty(P, x0, k, dt, discs, vel, w).sum(axis=-1) + (T + 1) * U * tot.astype(np.float64)
    return tot, bnd

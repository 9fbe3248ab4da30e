"""Extended-precision reference of the Euler rollout and of the cost, and the rounding bound of any fp64 evaluation of them
(test helper, CPU only; the conventions of update_reference.py).

From fp64 controls u [K][H-1][udim], the start state x0, dt, the window x_ref / y_ref [H], yaw_ref0 and an MPPIParams:

    yaw_t = yaw_0 + sum_{i<t} w_i dt             heading h_t = yaw_t (diff drive), yaw_t + u_t[2] (steering, full body)
    x_t = x_0 + sum_{i<t} v_i cos(h_i) dt        y_t likewise with sin                       X, Y [K][H]
    full body: roll_t, pitch_t like yaw_t from u[3], u[4]; zmp_y [K][H-2] by the closed form of
               tests/test_oracle.py::test_full_body_zmp_closed_form
    d_t = min(100, min_j |(x_t, y_t) - (x_ref_j, y_ref_j)|)                                   (the 100 m gate)
    diff drive, steering: cost = sum_{t<H} path_w d_t^2 + v_w (v_t - v_ref)^2,  v_{H-1} = 0.0 (the phantom control)
    full body: cost = yaw_w (yaw_0 - yaw_ref0)^2 + sum_{t<H-2} [path_w d_t^2 + v_w (v_t - v_ref)^2 + zmp_w zmp_y_t^2
               + roll_v_w (u_{t+1}[3] - u_t[3])^2 + (v_t < 0) back_w v_t^2],  zmp_w = roll_v_w = 0 with roll_off

all as real-number functions of the fp64 inputs: nothing on the way is rounded to fp64.

Arithmetic.  numpy.longdouble where it has a 64-bit mantissa (x87, nmant = 63).  A start angle is a double of any size up to
1e5, and a longdouble carries 1e5 only to 2^-47; so the start angle a_0 is reduced EXACTLY first: n = nearest integer to
a_0 / (pi/2) and r = a_0 - n pi/2 as a Fraction over a 330-bit pi (PI, checked against mpmath in the pinning test), r to
longdouble, sin / cos r by sinl / cosl, the quadrant from n.  Every later angle is a_0 + delta with |delta| a few radians,
accumulated in longdouble, and sin(a_0 + delta) = sin a_0 cos delta + cos a_0 sin delta.  Absolute error of every sine and
cosine a few 2^-64, of X, Y a few 2^-64 * (|x| + path length), pinned against mpmath at 240 bits in
test_rollout_reference.py.  Where longdouble is narrower the helper does NOT drop to fp64: backend "mp" evaluates the same
formulas with mpmath (80 bits; `backend="exact"`: 240 bits, which is what the pinning test compares against).

Rounding bounds (u = 2^-53), for ANY fp64 evaluation -- one that accumulates the angle and evaluates sin / cos of it each
step (the oracle, the plain kernel, steering, the wide-turn form), one that advances (sin, cos) by rotations (diff drive), or
one that does the first every few steps and the second in between (full body).  T = error of one sin / cos of a reduced
argument in units of u (an "ulp of 1": the spacing of doubles below 1).  Second-order terms (u^2) are dropped; every count
below is rounded up to make room for them.

  sin / cos of the heading at step j, eps_j (absolute):
      T u                          the evaluation itself (the seed of a rotation chain, or the evaluation at step j)
    + j u max(A + W, 6 + 2T + W)   per step, whichever is larger:
                                   accumulating: yaw <- fl(yaw + fl(w dt)) rounds by u |yaw| + u |w dt| <= u (A + W),
                                     A = max_t |yaw_t|, W = max_t |w_t dt| of the sample, and |d sin| <= |d angle|;
                                   rotating: (s, c) <- (s cd + c sd, c cd - s sd) is 4 products and 2 sums of magnitude
                                     <= 1 (6 u), 2 short polynomials (2 T u), and the rounded turn w dt (u W); a rotation
                                     does not enlarge the error it is handed, so the terms add up linearly
    + u max(|h_j|, 3 + 2T)         steering, full body: the rounded sum yaw + offset (u |h_j|), or the addition theorem
                                     on (sin, cos) of yaw and of the offset (2 products, 1 sum, 2 short polynomials)
  (roll and pitch: the same with their own A and W, no offset term.)

  position after t steps, bound_xy[k][t] (t = 0: the start position is copied, bound 0):
      sum_{i<t} |v_i dt| (eps_i + 2 u)    the trig error times the step; the two roundings of v c dt (or of v dt and the
                                          fused step * c + x: fewer)
    + (t + 1) u P_t                       t roundings of the running sum, one more for a change of origin (the kernels
                                          integrate relative to the start pose), P_t = max_{s<=t} max(|x_s|, |y_s|)

  cost, bound_cost[k]:
      path_w sum_t [2 d_t D_t + D_t^2]    D_t = sqrt 2 bound_xy[t] + dd_t: the distance to the nearest window point is
                                          1-Lipschitz in the position -- the minimum over the window of the perturbed
                                          distances moves by no more than the position does -- and so is min(100, .);
                                          d^2 moves by 2 d D + D^2
        dd_t = 4 u d_t + 8 u R_t^2 / max(d_t, sqrt(8 u) R_t)
                                          the evaluation of d_t itself: as sqrt of two squared differences (4 u d_t), or
                                          as |p|^2 + a_j p_x + b_j p_y + c_j relative to the start pose (8 roundings of
                                          terms <= R_t^2, R_t = |p_t - p_0| + max_j |r_j - p_0|: an absolute error of d^2,
                                          i.e. 8 u R^2 / d of d, and never more than sqrt(8 u) R where d is small)
    + sum_t v_w 4 u (v_t - v_ref)^2       difference, square, weight (and the reversing term likewise, 4 u back_w v^2;
                                          the roll-rate term 4 u roll_v_w (.)^2)
    + zmp_w sum_t [2 |z_t| Z_t + Z_t^2]   Z_t = [m L 9.8 eps_roll + m L (|a_y| (eps_roll + eps_pitch) + (|da| + |v w|) T u)
                                          + 14 u M_t] / 588: sin roll, cos pitch cos roll, sin / cos of the direction,
                                          and 14 roundings of terms bounded by M_t = the sum of the closed form's
                                          absolute terms
    + (3 H + 4) u cost                    the additions (at most 3 H + 1: every term is >= 0, every partial sum <= cost),
                                          the yaw term's 3 roundings

They are derived, not tuned.  test_rollout_reference.py shows the oracle (libm trig, rounded accumulation) inside them with
T = 1, and eleven wrong evaluations outside.

T.  measured_trig_ulps() takes it from step 0 of a rollout that starts at the origin: x_1 = fl(fl(v_0 cos h_0) dt) has two
roundings (with x_0 != 0 three: their allowance is subtracted), the rest of |x_1 - v_0 cos h_0 dt| / (u |v_0 dt|) is T,
rounded up to an integer >= 1.  T_MAX = 2 (csrc/fast_trig.h: "within 1 ulp ... 1.3 ulp"); more is a finding, not a tolerance.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
T_MAX = 2
LD = np.longdouble
HAVE_LD64 = np.finfo(LD).nmant >= 63
GATE = 100.0
# pi to 100 decimals (330 bits)
PI = Fraction(int("31415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679"),
              10 ** 100)
HALF_PI = PI / 2
FB_MASS, FB_HEIGHT, FB_WIDTH, FB_G = 60.0, 0.8075, 0.208, 9.8


def reduce_exact(a):
    """(n, r): n = nearest integer to a / (pi/2), r = a - n pi/2 as a Fraction (a: a double, taken exactly)."""
    fa = Fraction(float(a))
    q = fa / HALF_PI
    n = math.floor(q + Fraction(1, 2))
    return n, fa - n * HALF_PI


def _frac_to_ld(fr):
    """Fraction -> longdouble, to 2^-64 relative: the double nearest to it plus the double nearest to the rest"""
    hi = float(fr)
    lo = float(fr - Fraction(hi))
    return LD(hi) + LD(lo)


def sincos_exact_ld(a):
    """(sin a, cos a) as longdoubles, absolute error a few 2^-64, for a double a of any size"""
    n, r = reduce_exact(a)
    rl = _frac_to_ld(r)
    s, c = np.sin(rl), np.cos(rl)
    q = n % 4
    return [(s, c), (c, -s), (-s, -c), (-c, s)][q]


def _mp_sincos(a, prec):
    import mpmath
    with mpmath.workprec(prec):
        return mpmath.sin(mpmath.mpf(float(a))), mpmath.cos(mpmath.mpf(float(a)))


def fb_constants(F=LD):
    """(m, L, Ixx, m g) of the full-body model from the constants as the closed form writes them, in the arithmetic F"""
    m, h, w = F(FB_MASS), F(FB_HEIGHT), F(FB_WIDTH)
    L = h / 2
    return m, L, (m * (w * w + h * h)) / 12 + m * L * L, F(588.0)


class RolloutRef:
    """X, Y [K][H], costs [K] (longdouble), full body: roll, pitch [K][H], zmp_y [K][H-2]; and what the bounds need."""

    def __init__(self, p, u, x0, dt):
        self.p, self.u, self.dt = p, np.asarray(u, dtype=np.float64), float(dt)
        self.x0 = np.asarray(x0, dtype=np.float64)
        self.K, self.H = self.u.shape[0], self.u.shape[1] + 1

    # ---- bounds (fp64 arrays) ----
    def _eps(self, ang, rate_dt, T, offset_heading=None):
        """eps_j [K][H-1]: the error of sin / cos of an accumulated angle at control step j (module docstring)"""
        A = np.max(np.abs(ang), axis=1, keepdims=True)
        W = np.max(np.abs(rate_dt), axis=1, keepdims=True)
        j = np.arange(self.H - 1, dtype=np.float64)[None, :]
        e = T + j * (np.maximum(A + W, 6.0 + 2 * T + W))
        if offset_heading is not None:
            e = e + np.maximum(np.abs(offset_heading), 3.0 + 2 * T)
        return U * e

    def eps_heading(self, T=1):
        off = None if self.p.model == "diff_drive" else self.heading
        return self._eps(self.yaw, self.u[:, :, 1] * self.dt, T, off)

    def bound_xy(self, T=1):
        eps = self.eps_heading(T)
        vdt = np.abs(self.u[:, :, 0] * self.dt)
        grow = np.concatenate([np.zeros((self.K, 1)), np.cumsum(vdt * (eps + 2 * U), axis=1)], axis=1)
        P = np.maximum.accumulate(np.maximum(np.abs(self.X64), np.abs(self.Y64)), axis=1)
        t = np.arange(self.H, dtype=np.float64)[None, :]
        b = grow + (t + 1) * U * P
        b[:, 0] = 0.0
        return b

    def bound_cost(self, T=1):
        p, H = self.p, self.H
        fb = p.model == "full_body"
        n = H - 2 if fb else H
        bxy = self.bound_xy(T)[:, :n]
        d, R = self.d64[:, :n], self.R64[:, :n]
        dd = 4 * U * d + 8 * U * R * R / np.maximum(d, math.sqrt(8 * U) * R)
        D = math.sqrt(2.0) * bxy + dd
        b = p.path_weight * np.sum(2 * d * D + D * D, axis=1)
        v = self.v_cost[:, :n]
        b = b + 4 * U * p.v_weight * np.sum((v - p.v_ref) ** 2, axis=1)
        if fb:
            zw = 0.0 if p.roll_off else p.zmp_weight
            rw = 0.0 if p.roll_off else p.roll_v_weight
            u = self.u
            b = b + 4 * U * p.back_weight * np.sum(np.where(v < 0, v * v, 0.0), axis=1)
            b = b + 4 * U * rw * np.sum((u[:, 1:n + 1, 3] - u[:, :n, 3]) ** 2, axis=1)
            if zw:
                m, L, Ixx, mg = (float(c) for c in fb_constants())
                er = self._eps(self.roll, u[:, :, 3] * self.dt, T)[:, :n]
                ep = self._eps(self.pitch, u[:, :, 4] * self.dt, T)[:, :n]
                da = np.abs((u[:, 1:n + 1, 0] - u[:, :n, 0]) / self.dt)
                vw = np.abs(u[:, :n, 0] * u[:, :n, 1])
                ay = np.abs(self.ay64)
                M = (m * L * FB_G * np.abs(np.sin(self.roll[:, :n])) + m * L * (da + vw)
                     + Ixx * np.abs(u[:, 1:n + 1, 3] - u[:, :n, 3]) / abs(self.dt)) / mg
                Z = (m * L * FB_G * er + m * L * (ay * (er + ep) + (da + vw) * T * U)) / mg + 14 * U * M
                z = np.abs(self.zmp64)
                b = b + zw * np.sum(2 * z * Z + Z * Z, axis=1)
        return b + (3 * H + 4) * U * np.abs(self.costs64)

    # ---- comparisons ----
    def err_xy_over_bound(self, cand, T=1):
        """max |cand[k][t] - (X, Y)[k][t]| / bound_xy (cand [K][H][2]); the start position must be exact"""
        cand = np.asarray(cand, dtype=np.float64)
        ex = np.abs(cand[:, :, 0].astype(LD) - self.X).astype(np.float64)
        ey = np.abs(cand[:, :, 1].astype(LD) - self.Y).astype(np.float64)
        e = np.maximum(ex, ey)
        b = self.bound_xy(T)
        assert np.all(e[:, 0] == 0.0), "the start position is copied, not computed"
        return float(np.max(e[:, 1:] / b[:, 1:]))

    def err_cost_over_bound(self, costs, T=1):
        e = np.abs(np.asarray(costs, dtype=np.float64).astype(LD) - self.costs).astype(np.float64)
        return float(np.max(e / self.bound_cost(T)))

    def at_gate(self):
        """does any (sample, step) sit at the 100 m gate?  (a condition on the inputs of a test, not a measurement)"""
        return bool(np.any(self.d64 >= GATE))


def measured_trig_ulps(ref, cand):
    """T as the module docstring defines it, from step 0 -> 1 of the candidates [K][H][2]; the caller asserts T <= T_MAX."""
    cand = np.asarray(cand, dtype=np.float64)
    vdt = np.abs(ref.u[:, 0, 0] * ref.dt)
    live = vdt > 0
    if not live.any():
        return 1
    worst = -np.inf
    for got, want, trig in ((cand[:, 1, 0], ref.X[:, 1], ref.c0), (cand[:, 1, 1], ref.Y[:, 1], ref.s0)):
        err = np.abs(got.astype(LD) - want).astype(np.float64)
        moved = 0.0 if (ref.x0[0] == 0.0 and ref.x0[1] == 0.0) else 2 * U * np.abs(want.astype(np.float64))
        other = 2 * U * vdt * np.abs(trig) + moved
        if ref.p.model != "diff_drive":
            other = other + U * vdt * np.maximum(np.abs(ref.heading[:, 0]), 3.0 + 2 * T_MAX)
        worst = max(worst, float(np.max(((err - other) / (U * vdt))[live])))
    return max(1, int(math.ceil(worst)))


# ---- the reference itself -----------------------------------------------------------------------------------------------
def _angles_ld(a0, rate, dt):
    """delta [K][H] = sum_{i<t} rate_i dt in longdouble (delta_0 = 0); the angle itself is a0 + delta"""
    inc = rate.astype(LD) * LD(dt)
    return np.concatenate([np.zeros((rate.shape[0], 1), dtype=LD), np.cumsum(inc, axis=1)], axis=1)


def _sincos_from(a0, delta):
    s0, c0 = sincos_exact_ld(a0)
    sd, cd = np.sin(delta), np.cos(delta)
    return s0 * cd + c0 * sd, c0 * cd - s0 * sd


def reference(p, u, x0, dt, x_ref, y_ref, yaw_ref0, backend=None):
    backend = backend or ("longdouble" if HAVE_LD64 else "mp")
    if backend != "longdouble":
        return _reference_mp(p, u, x0, dt, x_ref, y_ref, yaw_ref0, 240 if backend == "exact" else 80)
    r = RolloutRef(p, u, x0, dt)
    u, x0 = r.u, np.zeros(5)
    x0[:len(r.x0)] = r.x0
    K, H, fb = r.K, r.H, p.model == "full_body"
    dtl = LD(dt)
    dyaw = _angles_ld(x0[2], u[:, :, 1], dt)
    off = np.zeros((K, H - 1), dtype=LD) if p.model == "diff_drive" else u[:, :, 2].astype(LD)
    s, c = _sincos_from(x0[2], dyaw[:, :H - 1] + off)
    v = u[:, :, 0].astype(LD)
    zero = np.zeros((K, 1), dtype=LD)
    r.X = LD(x0[0]) + np.concatenate([zero, np.cumsum(v * c * dtl, axis=1)], axis=1)
    r.Y = LD(x0[1]) + np.concatenate([zero, np.cumsum(v * s * dtl, axis=1)], axis=1)
    r.s0, r.c0 = s[:, 0].astype(np.float64), c[:, 0].astype(np.float64)
    r.yaw = (LD(x0[2]) + dyaw).astype(np.float64)
    r.heading = (LD(x0[2]) + dyaw[:, :H - 1] + off).astype(np.float64)
    xr, yr = np.asarray(x_ref, dtype=np.float64).astype(LD), np.asarray(y_ref, dtype=np.float64).astype(LD)
    dist = np.sqrt((r.X[:, :, None] - xr[None, None, :]) ** 2 + (r.Y[:, :, None] - yr[None, None, :]) ** 2)
    d = np.minimum(LD(GATE), np.min(dist, axis=2))
    r.v_cost = np.concatenate([u[:, :, 0], np.zeros((K, 1))], axis=1)          # the phantom control reads 0.0
    vc = r.v_cost.astype(LD)
    if not fb:
        cost = np.sum(LD(p.path_weight) * d * d + LD(p.v_weight) * (vc - LD(p.v_ref)) ** 2, axis=1)
    else:
        n = H - 2
        droll, dpitch = _angles_ld(x0[3], u[:, :, 3], dt), _angles_ld(x0[4], u[:, :, 4], dt)
        sr, cr = _sincos_from(x0[3], droll[:, :n])
        _, cp = _sincos_from(x0[4], dpitch[:, :n])
        r.roll, r.pitch = (LD(x0[3]) + droll).astype(np.float64), (LD(x0[4]) + dpitch).astype(np.float64)
        m, L, Ixx, mg = fb_constants()
        w, di = u[:, :n, 1].astype(LD), u[:, :n, 2].astype(LD)
        da = (v[:, 1:n + 1] - v[:, :n]) / dtl
        ay = da * np.sin(di) + v[:, :n] * w * np.cos(di)
        drv = u[:, 1:n + 1, 3].astype(LD) - u[:, :n, 3].astype(LD)
        r.zmp = (m * (LD(FB_G) * L * sr + L * cp * cr * ay) - Ixx * drv / dtl) / (-mg)
        r.ay64, r.zmp64 = ay.astype(np.float64), r.zmp.astype(np.float64)
        zw = LD(0.0 if p.roll_off else p.zmp_weight)
        rw = LD(0.0 if p.roll_off else p.roll_v_weight)
        vn = v[:, :n]
        terms = (LD(p.path_weight) * d[:, :n] ** 2 + LD(p.v_weight) * (vn - LD(p.v_ref)) ** 2 + zw * r.zmp ** 2
                 + rw * drv ** 2 + np.where(u[:, :n, 0] < 0.0, LD(p.back_weight) * vn * vn, LD(0)))
        cost = LD(p.yaw_weight) * (LD(x0[2]) - LD(yaw_ref0)) ** 2 + np.sum(terms, axis=1)
    r.d, r.costs = d, cost
    r.X64, r.Y64, r.d64, r.costs64 = (a.astype(np.float64) for a in (r.X, r.Y, d, cost))
    rel = np.sqrt((r.X64 - x0[0]) ** 2 + (r.Y64 - x0[1]) ** 2)
    far = float(np.max(np.sqrt((np.asarray(x_ref, dtype=np.float64) - x0[0]) ** 2 +
                               (np.asarray(y_ref, dtype=np.float64) - x0[1]) ** 2)))
    r.R64 = rel + far
    return r


def _reference_mp(p, u, x0_in, dt, x_ref, y_ref, yaw_ref0, prec):
    """the same formulas with mpmath at `prec` bits, sample by sample (slow; the pinning test's side and the fall-back)"""
    import mpmath
    r = RolloutRef(p, u, x0_in, dt)
    u = r.u
    x0 = np.zeros(5)
    x0[:len(r.x0)] = r.x0
    K, H, fb = r.K, r.H, p.model == "full_body"
    mp = mpmath.mpf
    out = {k: np.zeros((K, H), dtype=LD) for k in ("X", "Y")}
    costs, dmin = np.zeros(K, dtype=LD), np.zeros((K, H), dtype=LD)
    zmp, ayv = np.zeros((K, max(H - 2, 1)), dtype=LD), np.zeros((K, max(H - 2, 1)), dtype=LD)
    yaw, head = np.zeros((K, H)), np.zeros((K, H - 1))
    roll, pitch = np.zeros((K, H)), np.zeros((K, H))
    s0, c0 = np.zeros(K), np.zeros(K)
    with mpmath.workprec(prec):
        def ld(x):
            hi = float(x)
            return LD(hi) + LD(float(x - mp(hi)))
        dtm = mp(float(dt))
        xr, yr = [mp(float(a)) for a in x_ref], [mp(float(a)) for a in y_ref]
        m, L, Ixx, mg = fb_constants(mp)
        for k in range(K):
            x, y, a = mp(float(x0[0])), mp(float(x0[1])), mp(float(x0[2]))
            ro, pi_ = mp(float(x0[3])), mp(float(x0[4]))
            xs, ys, ros, pis = [x], [y], [ro], [pi_]
            yaw[k, 0] = float(a)
            for t in range(H - 1):
                ut = [mp(float(q)) for q in u[k, t]]
                h = a if p.model == "diff_drive" else a + ut[2]
                head[k, t] = float(h)
                ch, sh = mpmath.cos(h), mpmath.sin(h)
                if t == 0:
                    s0[k], c0[k] = float(sh), float(ch)
                x, y, a = x + ut[0] * ch * dtm, y + ut[0] * sh * dtm, a + ut[1] * dtm
                if fb:
                    ro, pi_ = ro + ut[3] * dtm, pi_ + ut[4] * dtm
                xs.append(x); ys.append(y); ros.append(ro); pis.append(pi_)
                yaw[k, t + 1] = float(a)
            ds = [min(mp(GATE), min(mpmath.sqrt((xs[t] - xr[j]) ** 2 + (ys[t] - yr[j]) ** 2) for j in range(H)))
                  for t in range(H)]
            vs = [mp(float(q)) for q in u[k, :, 0]] + [mp(0)]
            if not fb:
                c = sum(mp(p.path_weight) * ds[t] ** 2 + mp(p.v_weight) * (vs[t] - mp(p.v_ref)) ** 2 for t in range(H))
            else:
                zw = mp(0.0 if p.roll_off else p.zmp_weight)
                rw = mp(0.0 if p.roll_off else p.roll_v_weight)
                c = mp(p.yaw_weight) * (mp(float(x0[2])) - mp(float(yaw_ref0))) ** 2
                for t in range(H - 2):
                    ut, un = [mp(float(q)) for q in u[k, t]], [mp(float(q)) for q in u[k, t + 1]]
                    da = (un[0] - ut[0]) / dtm
                    ay = da * mpmath.sin(ut[2]) + ut[0] * ut[1] * mpmath.cos(ut[2])
                    z = (m * (mp(FB_G) * L * mpmath.sin(ros[t]) + L * mpmath.cos(pis[t]) * mpmath.cos(ros[t]) * ay)
                         - Ixx * (un[3] - ut[3]) / dtm) / (-mg)
                    zmp[k, t], ayv[k, t] = ld(z), ld(ay)
                    c += mp(p.path_weight) * ds[t] ** 2 + mp(p.v_weight) * (ut[0] - mp(p.v_ref)) ** 2 + zw * z ** 2
                    c += rw * (un[3] - ut[3]) ** 2
                    if u[k, t, 0] < 0.0:
                        c += mp(p.back_weight) * ut[0] ** 2
            for t in range(H):
                out["X"][k, t], out["Y"][k, t], dmin[k, t] = ld(xs[t]), ld(ys[t]), ld(ds[t])
                roll[k, t], pitch[k, t] = float(ros[t]), float(pis[t])
            costs[k] = ld(c)
    r.X, r.Y, r.d, r.costs = out["X"], out["Y"], dmin, costs
    r.s0, r.c0, r.yaw, r.heading = s0, c0, yaw, head
    r.v_cost = np.concatenate([u[:, :, 0], np.zeros((K, 1))], axis=1)
    if fb:
        r.roll, r.pitch, r.zmp, r.zmp64, r.ay64 = roll, pitch, zmp, zmp.astype(np.float64), ayv.astype(np.float64)
    r.X64, r.Y64, r.d64, r.costs64 = (a.astype(np.float64) for a in (r.X, r.Y, dmin, costs))
    rel = np.sqrt((r.X64 - x0[0]) ** 2 + (r.Y64 - x0[1]) ** 2)
    far = float(np.max(np.sqrt((np.asarray(x_ref, dtype=np.float64) - x0[0]) ** 2 +
                               (np.asarray(y_ref, dtype=np.float64) - x0[1]) ** 2)))
    r.R64 = rel + far
    return r


# ---- the inputs of the heading tests (shared by the CPU and the GPU test modules) ---------------------------------------
def hardest_multiples(count=32, n_max=63661):
    """The `count` doubles x = nearest double to n pi/2, n = 1 .. n_max, with the smallest |x - n pi/2|: (x, n, x - n pi/2 as
    a float), hardest first.  Integer / Fraction arithmetic on PI."""
    found = []
    for n in range(1, n_max + 1):
        x = float(n * HALF_PI)               # (a Fraction's float() is correctly rounded)
        found.append((abs(Fraction(x) - n * HALF_PI), x, n))
    found.sort()
    return [(x, n, float(Fraction(x) - n * HALF_PI)) for _, x, n in found[:count]]


_HARD = []


def hard_headings_from_above(count=4):
    """the `count` hardest doubles that lie ABOVE their multiple of pi/2 (the reduced argument is a tiny positive number)"""
    if not _HARD:
        _HARD.extend(hardest_multiples(64))
    return [x for x, n, r in _HARD if r > 0][:count]


def headings():
    q = math.pi / 4
    tie = []
    for s in (q, -q):
        lo1, hi1 = np.nextafter(s, -np.inf), np.nextafter(s, np.inf)
        tie += [float(np.nextafter(lo1, -np.inf)), float(lo1), s, float(hi1), float(np.nextafter(hi1, np.inf))]
    h = [0.3] + tie + [math.pi / 2, -math.pi / 2, 3 * q, -3 * q, math.pi, -math.pi, float(np.nextafter(math.pi, 4.0))]
    h += [2.5, -2.5, 100.0, -1234.5, 9.0e4, -9.0e4] + hard_headings_from_above(4)
    return h


def fast_trig_bound(p, theta, dt, roll=0.0, pitch=0.0):
    """The quantity the host compares with 1e5 (fast_trig_safe, csrc/ccv_mppi_capi.hip), in its fp64 operations."""
    umax = [max(abs(a), abs(b)) for a, b in zip(p.u_min, p.u_max)]
    steps = float(p.horizon - 1) * abs(dt)
    bound = abs(theta) + steps * umax[1]
    if p.model != "diff_drive":
        bound += umax[2]
    if p.model == "full_body":
        bound = max(bound, abs(roll) + steps * umax[3])
        bound = max(bound, abs(pitch) + steps * umax[4])
    return bound


def edge_headings(p, dt, roll=0.0, pitch=0.0, limit=1.0e5):
    """(theta_edge, the next double above): the largest start heading the host admits to the branch-free sin / cos, found
    from the formula of fast_trig_safe by stepping doubles, and the first one it does not."""
    umax = [max(abs(a), abs(b)) for a, b in zip(p.u_min, p.u_max)]
    t = limit - float(p.horizon - 1) * abs(dt) * umax[1] - (umax[2] if p.model != "diff_drive" else 0.0)
    while fast_trig_bound(p, t, dt, roll, pitch) <= limit:
        t = float(np.nextafter(t, np.inf))
    while not fast_trig_bound(p, t, dt, roll, pitch) <= limit:
        t = float(np.nextafter(t, -np.inf))
    return t, float(np.nextafter(t, np.inf))


def rotated_window(x_ref, y_ref, x0, y0, theta):
    """the window turned about (x0, y0) by theta (numpy, fp64: the result is an input like any other)"""
    c, s = math.cos(theta), math.sin(theta)
    dx, dy = np.asarray(x_ref) - x0, np.asarray(y_ref) - y0
    return x0 + c * dx - s * dy, y0 + s * dx + c * dy


# ---- a plain fp64 rollout with a pluggable sincos: the subject of the mutation tests ------------------------------------
def _libm_fma():
    import ctypes
    import ctypes.util
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fma.restype = ctypes.c_double
    lib.fma.argtypes = [ctypes.c_double] * 3
    return np.frompyfunc(lib.fma, 3, 1)


_FMA = []


def fma(a, b, c):
    if not _FMA:
        _FMA.append(_libm_fma())
    return np.asarray(_FMA[0](a, b, c), dtype=np.float64)


C1, C2, C3 = 1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624879595063154e-21


def spec_sincos(x, mutation=None):
    """csrc/fast_trig.h fast_sincos restated operation by operation on fp64 arrays (libm's fma), or one wrong version of it"""
    x = np.asarray(x, dtype=np.float64)
    fn = np.rint(x * 6.36619772367581382433e-01)
    if mutation == "pio2_float32":
        r = fma(-fn, float(np.float32(math.pi / 2)), x)
    else:
        r = fma(-fn, C1, x)
        if mutation != "no_second_constant":
            r = fma(-fn, C2, r)
        r = fma(-fn, C3, r)
    z = r * r
    ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08)
    ps = fma(z, ps, 2.75573137070700676789e-06)
    ps = fma(z, ps, -1.98412698298579493134e-04)
    ps = fma(z, ps, 8.33333333332248946124e-03)
    ps = fma(z, ps, -1.66666666666666324348e-01)
    sr = fma(z * r, ps, r)
    pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09)
    pc = fma(z, pc, -2.75573143513906633035e-07)
    pc = fma(z, pc, 2.48015872894767294178e-05)
    pc = fma(z, pc, -1.38888888888741095749e-03)
    pc = fma(z, pc, 4.16666666666666019037e-02)
    cr = fma(z, fma(z, pc, -0.5), 1.0)
    q = fn.astype(np.int64)
    if mutation == "abs_q":
        q = np.abs(q)
    odd = (q & 1) != 0
    if mutation == "swap_odd":
        odd = np.zeros_like(odd)   # (never exchanged: the sine stays the sine for odd q)
    sa, ca = np.where(odd, cr, sr), np.where(odd, sr, cr)
    s = np.where((q & 2) != 0, -sa, sa)
    cbit = (q & 2) if mutation == "cos_sign_q2" else ((q + 1) & 2)
    c = np.where(cbit != 0, -ca, ca)
    return s, c


def fp64_rollout(p, u, x0_in, dt, x_ref, y_ref, yaw_ref0, sincos=None, mutation=None):
    """The Euler rollout and the cost in plain numpy fp64, the heading accumulated and sin / cos taken of it each step (what
    the oracle does), with the sine / cosine of `sincos` and, optionally, one deliberate mistake -> (cand [K][H][2], costs)."""
    sincos = sincos or (lambda a: (np.sin(a), np.cos(a)))
    u = np.asarray(u, dtype=np.float64)
    x0 = np.zeros(5)
    x0[:len(x0_in)] = x0_in
    K, H, fb = u.shape[0], u.shape[1] + 1, p.model == "full_body"
    X, Y = np.zeros((K, H)), np.zeros((K, H))
    X[:, 0], Y[:, 0] = x0[0], x0[1]
    yaw, roll, pitch = np.full(K, x0[2]), np.full(K, x0[3]), np.full(K, x0[4])
    rolls, pitches = [roll.copy()], [pitch.copy()]
    for t in range(H - 1):
        h = yaw if (p.model == "diff_drive" or mutation == "no_offset") else yaw + u[:, t, 2]
        s, c = sincos(h)
        step = 1.0 if (mutation == "no_dt" and t == 3) else dt
        X[:, t + 1] = X[:, t] + u[:, t, 0] * c * step
        Y[:, t + 1] = Y[:, t] + u[:, t, 0] * s * step
        yaw = yaw + u[:, t, 1] * dt
        if fb:
            roll, pitch = roll + u[:, t, 3] * dt, pitch + u[:, t, 4] * dt
            rolls.append(roll.copy())
            pitches.append(pitch.copy())
    xr, yr = np.asarray(x_ref, dtype=np.float64), np.asarray(y_ref, dtype=np.float64)
    d = np.min(np.sqrt((X[:, :, None] - xr) ** 2 + (Y[:, :, None] - yr) ** 2), axis=2)
    if mutation != "no_gate":
        d = np.minimum(GATE, d)
    cost = np.zeros(K)
    if not fb:
        phantom = 0.1 if mutation == "phantom" else 0.0
        v = np.concatenate([u[:, :, 0], np.full((K, 1), phantom)], axis=1)
        for t in range(H):
            cost = cost + (p.path_weight * d[:, t] ** 2 + p.v_weight * (v[:, t] - p.v_ref) ** 2)
    else:
        m, L, Ixx, mg = (float(c) for c in fb_constants(np.float64))
        zw = 0.0 if p.roll_off else p.zmp_weight
        rw = 0.0 if p.roll_off else p.roll_v_weight
        cost = cost + p.yaw_weight * (x0[2] - yaw_ref0) ** 2
        for t in range(H - 2):
            v, w, di = u[:, t, 0], u[:, t, 1], u[:, t, 2]
            da = (u[:, t + 1, 0] - v) / dt
            ay = da * np.sin(di) + v * w * np.cos(di)
            drv = u[:, t + 1, 3] - u[:, t, 3]
            z = (m * (FB_G * L * np.sin(rolls[t]) + L * np.cos(pitches[t]) * np.cos(rolls[t]) * ay) - Ixx * drv / dt) / (-mg)
            if mutation == "roll_v_shift":
                drv = u[:, t + 2, 3] - u[:, t + 1, 3] if t + 2 < H - 1 else drv
            cost = cost + p.path_weight * d[:, t] ** 2
            cost = cost + p.v_weight * (v - p.v_ref) ** 2
            cost = cost + zw * z * z
            cost = cost + rw * drv * drv
            back = (v > 0.0) if mutation == "back_positive" else (v < 0.0)
            cost = cost + np.where(back, p.back_weight * v * v, 0.0)
    return np.stack([X, Y], axis=-1), cost


# ---- the cases of the heading tests ----------------------------------------------------------------------------------------
ROLL_PITCH = {"rp0": (0.0, 0.0), "rp1": (0.3, -0.2), "rp2": (50.0, -7.0), "flags": (0.3, -0.2)}
K_HEADING, SEED = 130, 77


def input_sets():
    """(model, H, dt, variant) of every input set of tests/test_gpu_heading.py (the kernel family changes no input)"""
    out = [("diff_drive", H, dt, None) for H in (17, 9) for dt in (0.1, 0.4)]
    out += [("steering_diff_drive", H, 0.1, None) for H in (17, 9)]
    out += [("full_body", H, 0.1, v) for H in (17, 9) for v in ("rp0", "rp1", "rp2", "flags")]
    return out


def params_of(model, H, dt, variant=None, K=K_HEADING):
    from ccv_mppi_path_tracker_amd import configs
    mk = {"diff_drive": configs.diff_drive_defaults, "steering_diff_drive": configs.steering_defaults,
          "full_body": configs.full_body_defaults}[model]
    p = mk(K, H).with_(dt=dt)
    return p.with_(roll_off=True, steer_off=True) if variant == "flags" else p


_BASE = {}


def case_inputs(p, variant, theta):
    """(state, x_ref, y_ref, yaw_ref0): the pose 5 cm beside the fourth pose of the oracle's path (sinusoid; full body:
    dkan) turned to heading theta, the window from there turned about the pose by theta, yaw_ref0 = theta - 0.1"""
    import helpers
    key = (p.model, p.horizon, p.dt)
    if key not in _BASE:
        path = helpers.oracle_path("dkan" if p.model == "full_body" else "sinusoid")
        s = np.zeros(p.nstate)
        s[:2] = path[0][3], path[1][3] + 0.05
        xr, yr, _ = helpers.oracle_window(p, path, s)
        _BASE[key] = (s, xr, yr)
    s, xr, yr = _BASE[key]
    s = s.copy()
    s[2] = theta
    if p.model == "full_body":
        s[3], s[4] = ROLL_PITCH[variant]
    wx, wy = rotated_window(xr, yr, s[0], s[1], theta)
    return s, wx, wy, theta - 0.1


def case_headings(p, variant):
    rp = ROLL_PITCH[variant] if p.model == "full_body" else (0.0, 0.0)
    return headings() + list(edge_headings(p, p.dt, *rp))

"""Cases, inputs and checkers of the disc-obstacle terms, static and moving (10g).

The discs are chosen on the CPU from the oracle's Philox rollouts (discs_for, moving_discs_for) so that the conditions the GPU
tests assert on their inputs hold; check_penalty and check_moving hold cost_on - cost_off of one handle against the penalty
that tests/obstacle_reference.py and tests/moving_obstacle_reference.py give for the states the device stored.  The last
part is the numpy restatement of the device spec of the static term (spec, ring; fma and fmin live in obstacle_reference.py)
that the two reference tests share and tests/edge_probe.py holds the device against bit for bit; the moving term's restatement
is moving_obstacle_reference.spec.

Used by tests/test_gpu_batch_obstacles.py and tests/test_gpu_batch_moving.py, which exercise the checkers, by the grid,
costmap, roll, scan and horizon-sweep tests for their discs, and by tests/horizon_sweep_inputs.py, whose CPU test
(tests/test_horizon_sweep_inputs_cpu.py) pins the conditions without a GPU.  tests/test_obstacle_reference.py pins spec.
"""
import math

import numpy as np

import helpers
import moving_obstacle_reference as MR
import obstacle_reference as OR

LD = np.longdouble
NS = (0, 1, 3, 4, 32)   # discs per instance, dealt round
W_OBS = 5.0

# (model, K, H, B, overrides, kernel, family): K = 1 000: 16 workgroups, 40 live lanes in the last; H = 15: the TAIL forms, six
# steps in the last block; H = 10: one step in the last block, the step-by-step tail; the one-wave family through the workgroup
# count; the wide form through dt; the plain family: in the tests, through a heading
CASES = [("diff_drive", 1000, 15, 5, {}, "r4"), ("diff_drive", 1000, 10, 5, {}, "r4"), ("diff_drive", 1000, 15, 5, {"dt": 0.4}, "r4w"),
         ("steering_diff_drive", 1000, 15, 5, {}, "r4"), ("steering_diff_drive", 1000, 10, 5, {}, "r4"),
         ("full_body", 128, 15, 5, {}, "r4"), ("full_body", 128, 10, 5, {}, "r4"),
         ("diff_drive", 82048, 15, 2, {}, "solo")]


def nstates(p):
    return p.horizon - 2 if p.model == "full_body" else p.horizon


def oracle_states(p, x0, dt, nom, seed, it):
    o = helpers.oracle_for(p)
    o.set_nominal(nom)
    o.sampling(int(seed), rng="philox", iteration=it)
    o.predict_States(x0, dt)
    return np.stack([o.states("x"), o.states("y")], axis=-1)[:, :nstates(p)]


# ---- static discs ---------------------------------------------------------------------------------------------------------

def first_disc(P, x0, cands):
    """the first candidate centre whose tuned radius -- the median over the samples of the closest approach of the states
    t >= 1 -- leaves the start outside and between 30 % and 70 % of the samples inside"""
    for c in cands:
        dm = np.min(np.hypot(P[:, 1:, 0] - c[0], P[:, 1:, 1] - c[1]), axis=1)
        r = float(np.median(dm))
        if r < 0.95 * np.hypot(x0[0] - c[0], x0[1] - c[1]) and 0.3 <= np.mean(dm < r) <= 0.7:
            return (c[0], c[1], r)
    raise AssertionError("no candidate centre gives a usable disc")


def discs_for(p, inputs, it=0, ns=NS):
    """[B] arrays (n_b, 3).  Disc 0 on a window point near the middle of the horizon (the nearest one that first_disc accepts;
    the end state of a sample as the fall-back), radius tuned on the oracle's rollouts.  The others: discs 1 and 3 of 2 cm on
    the end states of samples 1 and 3 (a few samples touch them), the rest on a ring around the start that no sample reaches
    (they exercise the loop, the minimum and the padding)."""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    out = []
    for b in range(len(dt)):
        n = ns[b % len(ns)]
        d = np.zeros((n, 3))
        if n:
            P = oracle_states(p, x0[b], dt[b], nom[b], seeds[b], it)
            mid = p.horizon // 2
            order = sorted(range(1, p.horizon), key=lambda j: abs(j - mid))
            d[0] = first_disc(P, x0[b], [(xr[b, j], yr[b, j]) for j in order] + [P[0, -1], P[1, -1]])
            reach = 1.5 * max(abs(p.u_min[0]), abs(p.u_max[0])) * dt[b] * p.horizon + 2.0
            for i in range(1, n):
                if i in (1, 3) and np.hypot(*(P[i, -1] - x0[b, :2])) > 0.1:
                    d[i] = (P[i, -1, 0], P[i, -1, 1], 0.02)
                else:
                    d[i] = (x0[b, 0] + reach * np.cos(i), x0[b, 1] + reach * np.sin(i), 0.3 + 0.02 * i)
        out.append(d)
    return out


def check_penalty(what, p, x0, discs, w, off, on, share=True):
    """states bit-equal; cost_on - cost_off within the checker's bound of the reference penalty of the read-back states"""
    assert on["xy"].tobytes() == off["xy"].tobytes(), what
    P = on["xy"][:, :nstates(p)]
    tot, bnd = OR.sample_penalty(P, x0[:2], discs, w)
    diff = on["c"].astype(LD) - off["c"].astype(LD)
    allowed = bnd + OR.bound_difference(on["c"], off["c"], p.horizon)
    ratio = float(np.max(np.abs(diff - tot).astype(np.float64) / np.maximum(allowed, 1e-300)))
    frac = float(np.mean(tot > 0))
    print("err/bound [obstacles] %s: %.3g  (share with a penalty %.2f, largest penalty %.3g)" % (what, ratio, frac, float(tot.max())))
    assert np.all(np.abs(diff - tot).astype(np.float64) <= allowed), (what, ratio)
    if share and len(discs) and w > 0:
        assert 0.10 <= frac <= 0.90, (what, frac)
    return tot


# ---- moving discs ---------------------------------------------------------------------------------------------------------

def first_moving_disc(P, x0, dt, v_ref, cands):
    """cands: (step j, centre at step j, unit normal of the path there).  The first whose disc -- at the centre at step j,
    moving at v_ref along the normal, radius the median over the samples of the closest approach of the states k >= 1 to the
    disc where it is at step k -- leaves the pose outside at step 0 and between 30 % and 70 % of the samples inside."""
    ks = np.arange(P.shape[1])
    for j, c, nrm in cands:
        v = v_ref * np.asarray(nrm)
        o = np.asarray(c) - v * (j * dt)
        ctr = o[None, :] + v[None, :] * (ks * dt)[:, None]
        dm = np.min(np.hypot(P[:, 1:, 0] - ctr[1:, 0], P[:, 1:, 1] - ctr[1:, 1]), axis=1)
        r = float(np.median(dm))
        if r < 0.95 * np.hypot(x0[0] - o[0], x0[1] - o[1]) and 0.3 <= np.mean(dm < r) <= 0.7:
            return (o[0], o[1], r), (v[0], v[1])
    raise AssertionError("no candidate gives a usable moving disc")


def moving_discs_for(p, inputs, it=0, ns=NS):
    """([B] arrays (n_b, 3), [B] arrays (n_b, 2)).  Disc 0: first_moving_disc over the window points nearest the middle of the
    horizon, crossing to the left for even b and to the right for odd b (the fall-back, where the samples do not follow the
    window -- full body here: a mid-horizon or end state of sample 0 or 1 in the window point's place).  Discs 1 and 3: 2 cm, on
    the end states of samples 1 and 3 at the last step, drifting; the rest on a ring no sample reaches, drifting at 0.5 m/s
    (they exercise the loop, the minimum and the polynomial)."""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs, vels = [], []
    for b in range(len(dt)):
        n = ns[b % len(ns)]
        d, v = np.zeros((n, 3)), np.zeros((n, 2))
        if n:
            P = oracle_states(p, x0[b], dt[b], nom[b], seeds[b], it)
            T = P.shape[1]
            mid = p.horizon // 2
            cands = []
            for j in sorted(range(2, T - 1), key=lambda j: abs(j - mid)):
                tx, ty = xr[b, j + 1] - xr[b, j - 1], yr[b, j + 1] - yr[b, j - 1]
                s = (1.0 if b % 2 == 0 else -1.0) / np.hypot(tx, ty)
                cands.append((j, (xr[b, j], yr[b, j]), (-ty * s, tx * s)))
            for i, j in ((0, mid), (1, mid), (0, T - 1), (1, T - 1)):   # the fall-back: a state of a sample, at its own step
                tx, ty = P[i, j] - P[i, j - 1]
                s = (1.0 if b % 2 == 0 else -1.0) / max(np.hypot(tx, ty), 1e-12)
                cands.append((j, tuple(P[i, j]), (-ty * s, tx * s)))
            d[0], v[0] = first_moving_disc(P, x0[b], dt[b], p.v_ref, cands)
            reach = 1.5 * max(abs(p.u_min[0]), abs(p.u_max[0])) * dt[b] * p.horizon + 2.0
            for i in range(1, n):
                if i in (1, 3) and np.hypot(*(P[i, -1] - x0[b, :2])) > 0.1:
                    v[i] = (0.3, -0.2)
                    d[i] = (P[i, -1, 0] - v[i, 0] * (T - 1) * dt[b], P[i, -1, 1] - v[i, 1] * (T - 1) * dt[b], 0.02)
                else:
                    d[i] = (x0[b, 0] + reach * np.cos(i), x0[b, 1] + reach * np.sin(i), 0.3 + 0.02 * i)
                    v[i] = (-0.5 * np.sin(i), 0.5 * np.cos(i))
        discs.append(d)
        vels.append(v)
    return discs, vels


def check_moving(what, p, x0, dt, discs, vels, w, off, sta, mov, share=True):
    """states bit-equal; cost_moving - cost_off within the checker's bound of the reference penalty of the read-back states; the
    shares the docstring of tests/test_gpu_batch_moving.py states"""
    assert mov["xy"].tobytes() == off["xy"].tobytes() == sta["xy"].tobytes(), what
    T = nstates(p)
    P, ks = mov["xy"][:, :T], np.arange(T)
    tot, bnd = MR.sample_penalty(P, x0[:2], ks, dt, discs, vels, w)
    diff = mov["c"].astype(LD) - off["c"].astype(LD)
    allowed = bnd + MR.bound_difference(mov["c"], off["c"], p.horizon)
    miss = np.abs(diff - tot).astype(np.float64)
    ratio = float(np.max(miss / np.maximum(allowed, 1e-300)))
    frac = float(np.mean(tot > 0))
    print("err/bound [moving] %s: %.3g  (share with a penalty %.2f, largest penalty %.3g)" % (what, ratio, frac, float(tot.max())))
    assert np.all(miss <= allowed), (what, ratio)
    if share and len(discs) and w > 0:
        assert 0.10 <= frac <= 0.90, (what, frac)
        stot, _ = OR.sample_penalty(P, x0[:2], discs, w)
        hit = tot > 0
        apart = float(np.mean(np.abs(tot - stot).astype(np.float64)[hit] > 10.0 * allowed[hit]))
        print("    moving and static reference penalty more than 10 bounds apart: %.2f of the penalised samples" % apart)
        assert apart >= 0.10, (what, apart)


# ---- the device spec of the static term, operation by operation -----------------------------------------------------------

fma, fmin = OR.fma, OR.fmin   # (their home is obstacle_reference.py: the moving spec, which this module imports, needs them too)


def spec(P, x0, discs, w, wrong=None, parts=False):
    """The device spec for states P [T][2] of one sample: (s [T], cost after the T fma's from 0.0); with `parts`
    (s [T], g [T], cost).  wrong: one mistake, by name -- "pose", "factor2", "r", "pad0", "sum", "outside" (pinned by
    tests/test_obstacle_reference.py), "gpos" (g = max(s, 0)), "nanmin" (a minimum that lets a NaN f through)."""
    discs = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    n = discs.shape[0]
    ab, cc = [], []
    for ox, oy, r in discs:
        dx, dy = (ox, oy) if wrong == "pose" else (ox - x0[0], oy - x0[1])
        k = -1.0 if wrong == "factor2" else -2.0
        ab.append((k * dx, k * dy))
        cc.append(fma(dx, dx, dy * dy) - (r if wrong == "r" else r * r))
    while len(ab) % 4:
        ab.append((0.0, 0.0))
        cc.append(0.0 if wrong == "pad0" else math.inf)
    s_out, g_out, cost = [], [], 0.0
    for X, Y in np.asarray(P, dtype=np.float64):
        px, py = float(X - x0[0]), float(Y - x0[1])
        p2 = fma(px, px, py * py)
        f = [fma(a, px, fma(b, py, c)) for (a, b), c in zip(ab, cc)]
        if n == 0:
            s_out.append(math.inf if px == px and py == py else math.nan)
            g_out.append(0.0)
            continue
        if wrong == "sum":
            g = 0.0
            for fj in f[:n]:
                sj = fj + p2
                g += max(-sj, 0.0) if sj == sj else 0.0
            s_out.append(math.nan)
            g_out.append(g)
            cost = fma(w, g, cost)
            continue
        m = math.inf
        for fj in f:
            m = OR.nanmin(m, fj) if wrong == "nanmin" else fmin(m, fj)
        s = m + p2
        s_out.append(s)
        if wrong == "outside":
            g = max(s, 0.0) if s == s and s < math.inf else 0.0
        elif wrong == "gpos":
            g = max(s, 0.0) if s == s else 0.0
        else:
            g = max(-s, 0.0) if s == s else 0.0   # v_max_f64(-s, 0): NaN -> 0
        g_out.append(g)
        cost = fma(w, g, cost)
    if parts:
        return np.array(s_out), np.array(g_out), cost
    return np.array(s_out), cost


def ring(rng, centre, radius, count, eps):
    """positions at distance radius + eps_i of the centre, eps_i spread over +-eps"""
    th = rng.uniform(0, 2 * np.pi, count)
    rr = radius + rng.uniform(-eps, eps, count)
    return np.stack([centre[0] + rr * np.cos(th), centre[1] + rr * np.sin(th)], axis=1)

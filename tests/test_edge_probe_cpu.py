"""CPU tests of tests/edge_probe.py: the conditions tests/test_gpu_batch_edges.py asserts on the device's states hold on the
oracle's Philox rollouts of the same cases (obstacle_cases.oracle_states in place of the stored states), and every wrong version
of the three specs changes the expected bits of a probe of every case it applies to.

What applies where.  "early", "late" and "local" are mistakes in tau: the moving term only, and "local" (the step inside the
block of eight) is the right step wherever a case covers no more than eight states (full body, H = 10).  "nanmin" needs a disc
whose f is NaN: the instance with 32 discs, which a batch of two has as well.  "pad0" (padding with c = 0, a phantom disc of
radius 0 at the pose) changes s wherever every real disc is farther than the pose, and never a cost: a phantom that is the
minimum has s = |p|^2 >= 0.  It is pinned as such.  "le_nx" needs a state with fx == n exactly: the dyadic map."""
import math
from fractions import Fraction

import numpy as np
import pytest

import batch_support as BS
import edge_probe as EP
import grid_reference as GR
import moving_obstacle_reference as MR
import obstacle_cases as OC
import obstacle_reference as OR

# the GPU test's cases with K cut to 1 000 (the one-wave case differs from the first in K and B: its batch of two is kept)
CASES = []
for model, K, H, B, over, fam in OC.CASES:
    c = (model, min(K, 1000), H, B, tuple(sorted(over.items())))
    if c not in CASES:
        CASES.append(c)
IDS = ["%s-H%d-B%d%s" % (c[0], c[2], c[3], "-wide" if c[4] else "") for c in CASES]
SCENES = {}


def scene(case, moving, alt=False):
    """per instance: the oracle's states under march_params, the discs single_state_discs puts on them, what the spec gives"""
    key = (case, moving, alt)
    if key in SCENES:
        return SCENES[key]
    model, K, H, B, over = case
    p = BS.MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**dict(over))
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    plist, ns, out = EP.march_params(p, B), EP.disc_counts(B), []
    for b in range(B):
        n = ns[b % len(ns)]
        P = OC.oracle_states(plist[b], x0[b], dt[b], nom[b], seeds[b], 0)
        ks = np.arange(P.shape[1])
        build = P[:64] if B < len(OC.NS) else P   # (the one-wave case: as the GPU test, from the first 64 samples)
        discs, vels, targets = EP.single_state_discs(build, x0[b], dt[b], n, moving, lead=EP.lead_of(B, n, alt) if n in (1, 3) else None)
        count, cost = EP.expected_bits(P, ks, x0[b], dt[b], discs, vels, EP.W_EDGE)
        out.append(dict(n=n, P=P, ks=ks, x0=x0[b], dt=dt[b], discs=discs, vels=vels, targets=targets, count=count, cost=cost))
    SCENES[key] = out
    return out


def whole_spec(s, i, wrong=None):
    """(count, cost) of sample i by the whole spec over the whole list"""
    count, cost = EP.expected_bits(s["P"], s["ks"], s["x0"], s["dt"], s["discs"], s["vels"], EP.W_EDGE, wrong=wrong, samples=[i])
    return int(count[i]), float(cost[i])


def test_helpers_do_what_they_say():
    p = BS.MODEL_DEFAULTS["full_body"](128, 15)
    q = EP.silent(p)
    assert (q.path_weight, q.v_weight, q.zmp_weight, q.roll_v_weight, q.back_weight, q.yaw_weight) == (0.0,) * 6
    m = EP.marching(p, 0.8)
    assert m.u_min[0] == m.u_max[0] == 0.8 and m.u_min[1:] == p.u_min[1:] and m.u_max[1:] == p.u_max[1:]
    assert EP.parked(p).u_max[0] == 0.0 and EP.parked(p).u_min[0] == 0.0
    assert EP.steps(15) == [3, 7, 8, 14] and EP.steps(10) == [3, 5, 7, 8, 9] and EP.steps(8) == [3, 4, 7] and EP.steps(13) == [3, 6, 7, 8, 12]
    assert EP.ulps(1.0, 2) == 1.0 + 2 ** -51 and EP.ulps(1.0, -1) == 1.0 - 2 ** -53 and EP.ulps(1.0, 0) == 1.0
    for j in range(40):
        v = EP.velocity(j)
        assert np.hypot(*v) >= 2.0 and min(abs(v)) > 0.5
    assert min(pl.u_min[0] * 0.1 for pl in EP.march_params(p, 5)) >= 0.04   # 4 cm per step at the smallest dt


def test_the_fast_fma_is_the_rational_one():
    """random operands, sums that cancel to the last bits (the edge of a disc), ties, zeros, huge and tiny factors, non-numbers"""
    rng = np.random.default_rng(5)
    trips = []
    for _ in range(4000):
        a, b = rng.normal() * 10.0 ** rng.integers(-8, 4), rng.normal() * 10.0 ** rng.integers(-8, 4)
        trips += [(a, b, rng.normal()), (a, b, -a * b), (a, b, float(np.nextafter(-a * b, 0.0))), (a, b, -a * b * (1 + 2.0 ** -30))]
    trips += [(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0), (3.0, 2.0 ** -53, 1.0), (1.0, 2.0 ** -53, 1.0), (0.1, 3.0, -0.30000000000000004),
              (0.0, 5.0, -0.0), (-0.0, 5.0, 2.5), (7.3, 0.0, 0.0), (1e308, 1e308, 0.0), (1e308, 10.0, -1e308), (-2e308, 0.5, math.inf),
              (1e-200, 1e-200, 1e-300), (5e-324, 0.5, 0.0), (1e99, 1e99, 1.7e308), (math.nan, 1.0, 1.0), (math.inf, 0.0, 1.0),
              (-math.inf, 2.0, math.inf), (2.0, 3.0, math.inf), (1e-101, 1e50, 1.0), (1e101, 1e-50, 1.0)]
    for a, b, c in trips:
        x, y = OR.fma(a, b, c), OR.fma_rational(a, b, c)
        assert np.float64(x).tobytes() == np.float64(y).tobytes() or (x != x and y != y), (a, b, c, x, y)
    assert OC.fma is OR.fma and OR.fma(0.1, 3.0, -0.30000000000000004) != 0.0 == 0.1 * 3.0 - 0.30000000000000004


@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_target_counts_its_own_state_alone(case, moving):
    """the conditions of the GPU test; the steps the targets cover; and the short cuts of expected_bits -- the sign from the
    float64 power, the g over the discs near the minimum -- give the whole spec's count and bits on every target"""
    model, K, H, B, over = case
    T = OC.nstates(BS.MODEL_DEFAULTS[model](K, H))
    pos = zero = 0
    seen = set()
    for alt in ((False, True) if B < len(OC.NS) else (False,)):
        for b, s in enumerate(scene(case, moving, alt)):
            what = "%s b=%d n=%d" % (case, b, s["n"])
            assert len(s["discs"]) == s["n"] and len(s["targets"]) == (s["n"] if s["n"] < 32 else 30)
            a, z = EP.conditions(what, s["count"], s["targets"], s["n"])
            pos, zero = pos + a, zero + z
            for i, k, kind, j in s["targets"]:
                seen.add(k)
                c, cost = whole_spec(s, i)
                assert c == s["count"][i] and np.float64(cost).tobytes() == np.float64(s["cost"][i]).tobytes(), (what, i, k, kind)
                _, g, chain = EP.spec_of(s["P"][i], s["ks"], s["x0"], s["dt"], s["discs"], s["vels"], EP.W_EDGE)
                assert np.count_nonzero(np.delete(g, k)) == 0, (what, i, k)
                if c == 1:
                    assert cost == OC.fma(EP.W_EDGE, g[k], 0.0) > 0.0
                else:
                    assert cost == 0.0 and math.copysign(1.0, cost) == 1.0
            if s["n"] == 32:   # the far discs: f is NaN for the states to one side of the pose, and nothing counts
                assert np.all(np.abs(s["discs"][30:, 0]) > 1e300)
    print("%s %s: grazing targets with g > 0: %d, with g == 0: %d; steps %s" % (case, "moving" if moving else "static", pos, zero, sorted(seen)))
    assert pos >= 1 and zero >= 1
    want = {0, 1, T - 1} | {k for b in range((T + 7) // 8) for k in (8 * b, 8 * b + 7) if k < T}
    assert want <= seen, (case, sorted(want - seen))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_moving_disc_is_at_its_place_at_its_own_step_alone(case):
    for s in scene(case, True):
        for i, k, kind, j in s["targets"]:
            for kk in (k - 1, k + 1):
                _, g, _ = MR.spec(s["P"][i, k:k + 1], [kk], s["x0"], s["dt"], s["discs"][j:j + 1], s["vels"][j:j + 1], EP.W_EDGE, parts=True)
                assert g[0] == 0.0, (case, i, k, kk, kind)


def caught(case, moving, wrong, ns=None):
    """the first target whose expected bits the wrong version changes: (instance, sample, step, kind) or None"""
    for b, s in enumerate(scene(case, moving)):
        if ns is not None and s["n"] not in ns:
            continue
        for i, k, kind, j in s["targets"]:
            if s["count"][i] > 1:
                continue
            _, cost = whole_spec(s, i, wrong)
            if np.float64(cost).tobytes() != np.float64(s["cost"][i]).tobytes():
                return b, i, k, kind
    return None


@pytest.mark.parametrize("moving,wrong", [(False, w) for w in EP.WRONG_STATIC] + [(True, w) for w in EP.WRONG_MOVING],
                         ids=["static-" + w for w in EP.WRONG_STATIC] + ["moving-" + w for w in EP.WRONG_MOVING])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_wrong_disc_spec_changes_a_targets_bits(case, moving, wrong):
    model, K, H, B, over = case
    T = OC.nstates(BS.MODEL_DEFAULTS[model](K, H))
    hit = caught(case, moving, wrong, ns=(32,) if wrong == "nanmin" else None)
    print("%s %s %s: %s" % (case, "moving" if moving else "static", wrong, hit))
    if wrong == "local" and T <= MR.KTU:
        assert hit is None   # (every covered step lies in the first block: the step inside the block is the step)
    else:
        assert hit is not None


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_padding_with_zero_shows_in_s_and_in_no_cost(case):
    diff_s = 0
    alts = (False, True) if case[3] < len(OC.NS) else (False,)   # (discs round the pose itself are nearer than the phantom)
    for s in [s for alt in alts for s in scene(case, False, alt)]:
        if s["n"] % 4 == 0:
            continue
        for i, k, kind, j in s["targets"]:
            s0, g0, c0 = OC.spec(s["P"][i], s["x0"], s["discs"], EP.W_EDGE, parts=True)
            s1, g1, c1 = OC.spec(s["P"][i], s["x0"], s["discs"], EP.W_EDGE, "pad0", parts=True)
            assert np.array_equal(g0, g1) and np.float64(c0).tobytes() == np.float64(c1).tobytes()   # (g: a zero of either sign)
            diff_s += int(s0.tobytes() != s1.tobytes())
    assert diff_s > 0


# ---- the grid probes --------------------------------------------------------------------------------------------------------
MAPS = EP.probe_maps()


def test_the_probe_maps_are_what_they_say():
    for g in MAPS:
        assert g.nx != g.ny and all(n & (n - 1) for n in (g.nx, g.ny))
        assert len(np.unique(g.cells)) == g.cells.size and g.outside not in g.cells
    g = MAPS[0]
    assert all(Fraction(v).denominator <= 8 for v in (g.ox, g.oy, g.resolution, g.inv))   # dyadic: every fx is exact
    for g in MAPS[1:]:
        assert all(Fraction(v).denominator > 2 ** 20 for v in (g.ox, g.oy, g.resolution))


@pytest.mark.parametrize("m", range(len(MAPS)))
def test_grid_probes_straddle_every_boundary_by_one_ulp(m):
    g = MAPS[m]
    P, names, pairs = EP.grid_probes(g)
    v, inside, idx = GR.lookup(g, P[:, 0], P[:, 1])
    assert len(pairs) == 8 and len(P) == 26
    for lo, hi, axis, bound in pairs:
        origin, n = ((g.ox, g.nx), (g.oy, g.ny))[axis]
        a, b = P[lo, axis], P[hi, axis]
        assert float(np.nextafter(a, math.inf)) == b, names[lo]
        assert EP._f(a, origin, g.inv) < bound <= EP._f(b, origin, g.inv), names[lo]
        assert P[lo, 1 - axis] == P[hi, 1 - axis]
        assert v[lo] != v[hi], names[lo]                      # cell against neighbouring cell, or cell against `outside`
        if bound in (0, n):
            assert inside[hi] == (bound == 0) and inside[lo] == (bound == n), names[lo]
        else:
            assert inside[lo] and inside[hi] and idx[hi] - idx[lo] == (1 if axis == 0 else g.nx), names[lo]
    by = dict(zip(names, range(len(P))))
    for ax in "xy":
        assert inside[by[ax + " origin"]] and not inside[by[ax + " tiny negative"]] and not inside[by[ax + " in (-1, 0)"]]
        assert not inside[by[ax + " 2^32 + 2.5"]] and not inside[by[ax + " 1e300"]]
        k = by[ax + " 2^32 + 2.5"]
        f = EP._f(P[k, "xy".index(ax)], (g.ox, g.oy)["xy".index(ax)], g.inv)
        assert 4.0e9 < f < 4.4e9 and 0 <= int(GR._wrap32(np.trunc(np.float64(f)))) < min(g.nx, g.ny)
    # the numpy lookup the probes were made with is the exact one
    for k in range(len(P)):
        ve, ine, idxe = GR.lookup_exact(g, P[k, 0], P[k, 1])
        assert (np.float32(ve).tobytes(), bool(ine), int(idxe)) == (v[k].tobytes(), bool(inside[k]), int(idx[k])), names[k]


@pytest.mark.parametrize("wrong", GR.WRONG_LOOKUPS)
@pytest.mark.parametrize("m", range(len(MAPS)))
def test_every_wrong_lookup_changes_a_probes_value(m, wrong):
    """... and with it the expected cost: G is the covered states' sum of one value, fma(w, G, cost_off) with w > 0"""
    g = MAPS[m]
    P, names, pairs = EP.grid_probes(g)
    v, _, _ = GR.lookup(g, P[:, 0], P[:, 1])
    vw, _, _ = GR.lookup(g, P[:, 0], P[:, 1], wrong)
    hits = [names[k] for k in range(len(P)) if v[k].tobytes() != vw[k].tobytes()]
    print("map %d %s: %s" % (m, wrong, hits))
    exact_edge = any(EP._f(P[hi, axis], (g.ox, g.oy)[axis], g.inv) == bound for lo, hi, axis, bound in pairs if bound in (g.nx, g.ny))
    if wrong == "le_nx" and not exact_edge:
        assert not hits   # (no state has fx == n on this map: <= and < agree on every double)
    else:
        assert hits
        T = 15
        for k in (names.index(h) for h in hits):
            G, Gw = GR.grid_sum(g, np.tile(P[k], (1, T, 1))), GR.grid_sum(g, np.tile(P[k], (1, T, 1)), wrong)
            assert GR.fma(0.01, G[0], 3.7) != GR.fma(0.01, Gw[0], 3.7)
    if m == 0:
        assert exact_edge

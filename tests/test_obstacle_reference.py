"""Pins tests/obstacle_reference.py: a numpy restatement of the device spec of the disc-obstacle term,
fp64 operation by operation with an exactly rounded fma, lies inside the reference's bounds -- at states within 1e-9 m of a
disc's edge, 100 m away, for n in {0, 1, 3, 4, 32}, a NaN state and w_obs = 0 -- and seven wrong versions lie outside."""
import math

import numpy as np
import pytest

import obstacle_reference as OR
from obstacle_cases import fma, ring, spec

LD = np.longdouble


def scene(n, seed, far=False):
    rng = np.random.default_rng(seed)
    x0 = np.array([37.25, -12.5]) + rng.uniform(-1, 1, 2)
    discs = np.zeros((n, 3))
    discs[:, :2] = x0 + rng.uniform(-6, 6, (n, 2)) + (100.0 if far else 0.0)
    discs[:, 2] = rng.uniform(0.2, 1.5, n)
    parts = [x0 + rng.uniform(-8, 8, (24, 2)), x0[None, :]]
    for j in range(min(n, 3)):
        parts.append(ring(rng, discs[j, :2], discs[j, 2], 6, 1e-9))     # the edge: a difference of large numbers
        parts.append(ring(rng, discs[j, :2], 0.5 * discs[j, 2], 4, 0.1))  # well inside
    parts.append(x0 + 100.0 * np.array([[1.0, 0.3], [-0.7, 0.9]]))        # 100 m away
    return x0, discs, np.concatenate(parts)


CASES = [(n, far) for n in (0, 1, 3, 4, 32) for far in (False, True)]


@pytest.mark.parametrize("n,far", CASES)
def test_spec_inside_the_bounds(n, far):
    x0, discs, P = scene(n, 100 + n, far)
    w = 7.5
    s, cost = spec(P, x0, discs, w)
    ref_s = OR.power(P, discs)
    if n == 0:
        assert np.all(np.isinf(ref_s)) and cost == 0.0 and np.all(OR.penalty(P, discs, w) == 0)
        return
    err = np.abs(s.astype(LD) - ref_s).astype(np.float64)
    bnd = OR.bound_s(P, x0, discs)
    print("n=%d far=%s  max err/bound of s: %.3g" % (n, far, float(np.max(err / bnd))))
    assert np.all(err <= bnd)
    if not far:   # (the conditions: some states penetrate, some within 1e-9 m of an edge on either side)
        assert 4 <= np.count_nonzero(ref_s < 0) < len(P)
        assert np.count_nonzero((np.abs(ref_s) < 1e-8)) >= 4
    tot, tb = OR.sample_penalty(P[None], x0, discs, w)
    assert abs(LD(cost) - tot[0]) <= tb[0], (cost, tot[0], tb[0])
    # the bound is tight enough to mean something: a relative 1e-12 of the scale
    assert np.all(bnd <= 1e-14 * 100 * OR.scale(P, x0, discs))


def test_longdouble_and_exact_backends_agree():
    x0, discs, P = scene(4, 5)
    a, b = OR.power(P, discs), OR.power(P, discs, backend="exact")
    assert np.all(np.abs(a - b) <= OR.REF_ULPS * 2.0 ** -64 * OR.scale(P, x0, discs))
    np.testing.assert_array_equal(OR.penalty(P, discs, 0.0), np.zeros(len(P)))


def test_nan_state_and_zero_weight():
    x0, discs, P = scene(3, 9)
    P = np.concatenate([P, [[np.nan, 1.0], [2.0, np.nan], [np.nan, np.nan]]])
    s, cost = spec(P, x0, discs, 3.0)
    assert np.all(np.isnan(s[-3:])) and math.isfinite(cost)
    pen = OR.penalty(P, discs, 3.0)
    assert np.all(pen[-3:] == 0) and np.all(OR.bound_penalty(P, x0, discs, 3.0)[-3:] == 0)
    tot, tb = OR.sample_penalty(P[None], x0, discs, 3.0)
    assert abs(LD(cost) - tot[0]) <= tb[0]
    # w_obs = 0: fma(0, g, cost) = cost exactly
    _, c0 = spec(P, x0, discs, 0.0)
    assert c0 == 0.0 and OR.sample_penalty(P[None], x0, discs, 0.0)[0][0] == 0


@pytest.mark.parametrize("wrong", ["r", "sum", "factor2", "pose", "outside", "pad0", "no_relu"])
def test_wrong_versions_are_outside(wrong):
    """r instead of r^2; the sum over the discs instead of the deepest one; a missing factor 2 in a, b; the pose not
    subtracted; the penalty on s > 0; padding with c = 0 (a phantom disc of radius 0 at the pose: it never penetrates, so it
    shows in s -- wherever every real disc is farther than the pose -- and not in the penalty); w * (-s) without the maximum."""
    x0, discs, P = scene(3, 21)
    discs[1, :2] = discs[0, :2] + 0.3 * discs[0, 2]   # two discs overlap: a state inside both is charged once
    P = np.concatenate([P, ring(np.random.default_rng(3), discs[0, :2], 0.2 * discs[0, 2], 6, 0.01)])
    w = 7.5
    ref_s = OR.power(P, discs)
    tot, tb = OR.sample_penalty(P[None], x0, discs, w)
    if wrong == "no_relu":
        s, _ = spec(P, x0, discs, w)
        cost = 0.0
        for v in s:
            cost = fma(w, -v, cost)
    else:
        s, cost = spec(P, x0, discs, w, wrong)
    bad_cost = abs(LD(cost) - tot[0]) > tb[0]
    with np.errstate(invalid="ignore"):
        bad_s = bool(np.any(np.abs(s.astype(LD) - ref_s).astype(np.float64) > OR.bound_s(P, x0, discs)))
    if wrong == "pad0":
        assert bad_s and not bad_cost
    else:
        assert bad_cost, (wrong, cost, tot[0], tb[0])
    # ... and the right one is inside, on the same scene
    s, cost = spec(P, x0, discs, w)
    assert abs(LD(cost) - tot[0]) <= tb[0]
    assert np.all(np.abs(s.astype(LD) - ref_s).astype(np.float64) <= OR.bound_s(P, x0, discs))


def test_bound_difference_covers_reordered_sums():
    """two running sums of the same non-negative terms in different orders, one with the penalties fused in"""
    rng = np.random.default_rng(11)
    H = 15
    terms = rng.uniform(0, 50, 2 * H)
    pens = rng.uniform(0, 1e3, H)
    off = 0.0
    for t in terms:
        off += t
    on = 0.0
    for i in range(H):
        on = on + terms[2 * i + 1]
        on = on + terms[2 * i]
        on = fma(1.0, pens[i], on)
    real = math.fsum(pens)
    assert abs((on - off) - real) <= OR.bound_difference(on, off, H)
    assert OR.bound_difference(on, off, H) < 1e-9

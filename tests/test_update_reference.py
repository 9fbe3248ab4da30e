"""CPU tests (-m "not gpu") of tests/update_reference.py, the checker that test_gpu_update.py holds the HIP update against.

Why the checker exists: at the reference's lambda = 1 the softmax is so peaked that u* is decided by one to thirty samples,
and a lost ragged tail or a lost block of 64 samples moves u* by ~1e-16 -- far below the 1e-9 of the parity tests
(test_lambda_one_hides_a_lost_tail pins that).  With lambda chosen so that every sample carries weight (flat, graded) each
single sample moves u* by thousands of rounding bounds, and every mutation below must then fail the comparison.
"""
import numpy as np
import pytest

import helpers
import update_reference as R
from ccv_mppi_path_tracker_amd import configs

MODEL_CASES = [("C2", 4097, 17), ("C3", 1000, 15), ("C4", 130, 9)]   # one per model
_DATA = {}


def oracle_data(wl, K, H, lam=None, seed=42, iteration=7):
    """(params, costs, controls, u* of the fp64 oracle at `lam`) -- start 0.05 m beside the path; the costs do not depend on
    lambda."""
    key = (wl, K, H, lam)
    if key not in _DATA:
        w = configs.workload(wl, num_samples=K, horizon=H)
        p = w.params if lam is None else w.params.with_(lam=lam)
        path = helpers.oracle_path(w.path)
        state = np.zeros(p.nstate)
        state[0], state[1] = path[0][0], path[1][0] + 0.05
        xr, yr, yaw = helpers.oracle_window(p, path, state)
        o = helpers.oracle_for(p)
        u = o.iterate(state, p.dt, xr, yr, yaw[0], seed=seed, rng="philox", iteration=iteration)
        _DATA[key] = (p, o.costs(), o.get_controls(), u, o.sum_w())
    return _DATA[key]


def lam_of(costs, regime):
    return 1.0 if regime == "one" else R.regime_lambda(costs, regime)


def test_longdouble_is_wide_or_the_fallback_is_taken():
    assert R.HAVE_LD64 == (np.finfo(np.longdouble).nmant >= 63)
    acc = R.Accumulator(1.0)
    assert acc.backend == ("longdouble" if R.HAVE_LD64 else "exact80")


@pytest.mark.parametrize("wl,K,H", [("C2", 64, 9), ("C3", 33, 6), ("C4", 17, 5)])
@pytest.mark.parametrize("regime", ["flat", "graded", "one"])
def test_reference_against_exact_rational_arithmetic(wl, K, H, regime):
    """Fractions of the fp64 inputs, exp by mpmath at 400 bits (> 100 digits): S within 2^-58 relative, V and u_ref within
    2^-58 of their scale A (A / S) -- the scale the rounding bound is stated in; a row may cancel to nothing."""
    p, c, u, _, _ = oracle_data(wl, K, H)
    lam = lam_of(c, regime)
    shift = float(c.min()) if regime == "one" else 0.0      # (and the shifted form once)
    ref = R.reference(c, u, lam, shift)
    ex = R.Accumulator(lam, shift, backend="exact").add(c, u)
    tol = 2.0 ** -58
    assert abs(R._to_ld(ex.S) - ref.S) <= tol * ref.S
    A = np.array([R._to_ld(a) for a in ex.A])
    V = np.array([R._to_ld(v) for v in ex.V])
    uu = np.array([R._to_ld(v) for v in ex.exact_u()])
    assert np.all(np.abs(V - ref.V) <= tol * A)
    assert np.all(np.abs(uu - ref.u) <= tol * A / ref.S)
    assert np.all(np.abs(A - ref.A) <= tol * A)
    # the 80-bit fallback of hosts without a wide longdouble gives the same
    fb = R.reference(c, u, lam, shift, backend="exact80")
    assert np.all(np.abs(fb.u - uu) <= tol * A / ref.S) and abs(fb.S - ref.S) <= tol * ref.S


@pytest.mark.parametrize("wl,K,H", MODEL_CASES)
@pytest.mark.parametrize("regime", ["flat", "graded", "one"])
def test_fp64_oracle_passes_the_bound(wl, K, H, regime):
    _, c, _, _, _ = oracle_data(wl, K, H)
    lam = lam_of(c, regime)
    p, c2, u, u_o, s_o = oracle_data(wl, K, H, lam=lam)
    np.testing.assert_array_equal(c, c2)
    ref = R.reference(c, u, lam)
    r = ref.err_over_bound(u_o, E=1)
    print("oracle err/bound %s K=%d %s: %.2e" % (wl, K, regime, r))
    assert r <= 1.0
    assert abs(np.longdouble(s_o) - ref.S) <= ref.bound_S(E=1)
    w = np.exp(-c / lam)
    assert R.check_weights(c, lam, w, E=1) <= 1.0
    assert R.measured_exp_ulps(c, lam, w) <= R.E_MAX
    # and the same sums in another order
    u2, S2, _ = R.fp64_update(c[::-1], u[::-1], lam)
    assert ref.err_over_bound(u2) <= 1.0


def mutations(c, u, lam, swap):
    """name -> mutated fp64 result of the update"""
    K = len(c)
    u2 = u.reshape(K, -1)
    good, S, w = R.fp64_update(c, u2, lam)
    out = {}
    out["last sample dropped"] = R.fp64_update(c[:-1], u2[:-1], lam)[0]
    keep = np.arange(K) % 64 != 63
    out["lane 63 of every block of 64 dropped"] = R.fp64_update(c[keep], u2[keep], lam)[0]
    j = K // 3
    out["one sample counted twice"] = R.fp64_update(np.append(c, c[j]), np.vstack([u2, u2[j:j + 1]]), lam)[0]
    k = next(i for i in range(K // 2, K - 1) if swap[i] >= 100.0)     # (a pair that meets the input condition)
    us = u2.copy()
    us[[k, k + 1]] = us[[k + 1, k]]
    out["controls of samples k and k+1 swapped"] = R.fp64_update(c, us, lam)[0]
    row = good.copy()
    row[0] = row[1]
    out["row n taken from row n+1"] = row
    lo = min(64, K // 2)
    V = good * S
    out["one chunk partial left out of S only"] = V / (S - np.sum(w[lo:lo + 64]))
    return good, out


@pytest.mark.parametrize("wl,K,H", MODEL_CASES + [("C2", 65536, 50)])
@pytest.mark.parametrize("regime", ["flat", "graded"])
def test_the_checker_catches_every_mutation(wl, K, H, regime):
    p, c, u, _, _ = oracle_data(wl, K, H)
    lam = lam_of(c, regime)
    ref = R.reference(c, u, lam)
    drop, swap = R.sensitivities(c, u, ref)
    print("%s K=%d %s: min drop sensitivity %.3g, pairs below 100: %.3f %%" %
          (wl, K, regime, drop.min(), 100 * np.mean(swap < 100)))
    assert R.sensitivity_ok(drop, swap)
    good, muts = mutations(c, u, lam, swap)
    assert ref.err_over_bound(good) <= 1.0
    for name, bad in muts.items():
        assert ref.err_over_bound(bad) > 1.0, name


def test_lambda_one_hides_a_lost_tail():
    """The documented reason for this file: C2, K = 4097, H = 17 at the reference's lambda = 1 -- dropping the last sample (the
    ragged tail test_ragged_sample_counts exists for) and dropping the whole last block of 64 both move u* by less than the
    existing tests' 1e-9, so those tests cannot see either; the sensitivity condition correctly refuses this regime.
    (Blocks are the workgroups' blocks of 64 sample ids: at K = 4097 the last one, ids 4096 .. 4159, holds the tail alone.)"""
    p, c, u, _, _ = oracle_data("C2", 4097, 17)
    u2 = u.reshape(len(c), -1)
    good = R.fp64_update(c, u2, 1.0)[0]
    not_last_block = np.arange(len(c)) // 64 != (len(c) - 1) // 64
    assert helpers.rel_err(R.fp64_update(c[:-1], u2[:-1], 1.0)[0], good) < 1e-9
    assert helpers.rel_err(R.fp64_update(c[not_last_block], u2[not_last_block], 1.0)[0], good) < 1e-9
    ref = R.reference(c, u, 1.0)
    assert not R.sensitivity_ok(*R.sensitivities(c, u, ref))
    # ... while in the flat regime the same two losses are thousands of bounds
    lam = R.regime_lambda(c, "flat")
    ref = R.reference(c, u, lam)
    assert ref.err_over_bound(R.fp64_update(c[:-1], u2[:-1], lam)[0]) > 100.0
    assert ref.err_over_bound(R.fp64_update(c[:-64], u2[:-64], lam)[0]) > 100.0


def test_weight_check_and_zero_range_on_underflowing_weights():
    """Subnormal handling: weights that underflow are bracketed, not required bit for bit."""
    c = np.array([10.0, 700.0, 744.0, 744.5, 745.2, 746.0, 800.0])
    w = np.exp(-c)
    assert R.check_weights(c, 1.0, w, E=1) <= 1.0
    must, may = R.zero_count_range(c, 1.0, E=1)
    # 2^-1074 = exp(-744.44), 2^-1075 = exp(-745.13): 744.5 may go either way, 745.2 and beyond must be 0
    assert must <= int((w == 0).sum()) <= may and (must, may) == (3, 4)
    bad = w.copy()
    bad[1] *= 1 + 1e-12
    assert R.check_weights(c, 1.0, bad, E=1) > 1.0


def test_accumulating_in_slices_equals_one_pass():
    p, c, u, _, _ = oracle_data("C3", 1000, 15)
    lam = R.regime_lambda(c, "graded")
    one = R.reference(c, u, lam)
    acc = R.Accumulator(lam)
    for a in range(0, 1000, 300):
        acc.add(c[a:a + 300], u[a:a + 300])
    two = acc.finish()
    assert two.K == 1000 and abs(two.S - one.S) <= 2.0 ** -60 * one.S
    assert np.all(np.abs(two.u - one.u) <= 2.0 ** -58 * one.A / one.S)

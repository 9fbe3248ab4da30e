"""The two checkers of the weighted update u* = sum w_k u_k / sum w_k, and what their callers need to feed them.

check_update (plain weights and MIN_SHIFT on single handles; tests/test_gpu_update.py states its bound) and check_shift (the
batch handles' shifted-weight mode; tests/test_gpu_batch_shift.py derives E_SHIFT) stand side by side: each forms the
extended-precision reference of tests/update_reference.py from the device's own read-backs, holds the weights to its own
bound, and hands u*, sum_w, the statistics and the conditions on the inputs to one common tail, check_tail.  Beside them: the
batch inputs of the update tests, the sample controls rebuilt on the host, the lambdas dealt per instance, and the switch of
CCV_MPPI_KERNEL.

pytest rewrites no assert of a plain module, so every assert here names its case and the values it compares.  The checkers
are exercised by tests/test_gpu_update.py and tests/test_gpu_batch_shift.py, the reference by tests/test_update_reference.py.
"""
import math

import numpy as np

import helpers
import update_reference as R
from batch_support import instance_seed

LD = np.longdouble
E_SHIFT = 2 * R.E_MAX + 1


def report(group, what, ratio):
    print("err/bound [%s] %s: %.3g" % (group, what, ratio))


def check_tail(group, label, what, ref, E, costs, controls, lam, shift, u_dev, sum_w, stats, sens):
    """What check_update and check_shift assert alike, with the checker's E: u* against the reference's bound (printed under
    `label`), sum_w against bound_S, min / max cost and the flag exactly, the zero-weight count inside its range, and from
    K = 64 up the conditions on the inputs: losing any one sample moves u* by >= 100 bounds, pairing a sample's weight with its
    neighbour's controls does for >= 99 % of the pairs."""
    K = len(costs)
    ratio = ref.err_over_bound(u_dev, E)
    report(group, label, ratio)
    assert ratio <= 1.0, (what, ratio)
    if sum_w is not None:
        assert abs(LD(sum_w) - ref.S) <= ref.bound_S(E), (what, sum_w, ref.S, ref.bound_S(E))
    if stats is not None:
        assert stats.min_cost == costs.min() and stats.max_cost == costs.max() and stats.nonfinite == 0, (
            what, stats.min_cost, costs.min(), stats.max_cost, costs.max(), stats.nonfinite)
        must, may = R.zero_count_range(costs, lam, E, shift)
        assert must <= stats.n_zero_weight <= may, (what, must, stats.n_zero_weight, may)
    if sens and K >= 64:
        drop, swap = R.sensitivities(costs, controls, ref, E)
        assert drop.min() >= 100.0, (what, drop.min())
        assert np.mean(swap >= 100.0) >= 0.99, (what, np.mean(swap < 100.0))


def check_update(group, what, costs, controls, lam, u_dev, sum_w=None, w_norm=None, stats=None, shift=0.0, sens=True):
    """Everything the docstring of tests/test_gpu_update.py lists, from the device's own arrays.  Returns the reference.
    sum_w None (enqueue-only paths return no statistics: exchange, resident ticks): E cannot be separated from the error of
    the device's S there, so E is its cap E_MAX and the normalised weights are held against w_ref / S_ref with the bound of S,
    (K + 1 + X + E) u, added to theirs."""
    K = len(costs)
    ref = R.reference(costs, controls, lam, shift)
    E = R.E_MAX if sum_w is None else 1
    if w_norm is not None:
        w_norm = np.asarray(w_norm)
        if sum_w is not None:
            w_dev = w_norm * sum_w
            E = R.measured_exp_ulps(costs, lam, w_dev, shift)
            assert E <= R.E_MAX, "%s: device exp off by %d ulp" % (what, E)
            rw = R.check_weights(costs, lam, w_dev, E, shift)
            assert rw <= 1.0, (what, rw)
        else:
            w_ref, x, _ = R.weight_errors(costs, lam, w_norm, shift)
            allowed = (np.abs(x) + 2 * E + 2 + K + 1 + ref.xmax + E) * R.U * (w_ref / ref.S).astype(np.float64)
            miss = np.abs(w_norm - (w_ref / ref.S).astype(np.float64))
            assert np.all(miss <= np.maximum(allowed, R.TINY * (E + 1))), (what, float(np.max(miss)), float(np.max(allowed)))
        assert abs(math.fsum(w_norm) - 1.0) <= K * R.U, (what, math.fsum(w_norm), K * R.U)
    check_tail(group, what, what, ref, E, costs, controls, lam, shift, u_dev, sum_w, stats, sens)
    if stats is not None and w_norm is not None and sum_w <= 1.0:     # (w / S cannot underflow where w did not)
        assert stats.n_zero_weight == int((w_norm == 0).sum()), (what, stats.n_zero_weight, int((w_norm == 0).sum()))
    return ref


def check_shift(what, costs, controls, lam, u_dev, sum_w=None, w_norm=None, stats=None, sens=True):
    """Check 1 of the docstring of tests/test_gpu_batch_shift.py for one instance.  sum_w None (resident ticks return no
    statistics): the normalised weights are held against w_ref / S_ref with the bound of S added to theirs, as check_update
    does."""
    K, E = len(costs), E_SHIFT
    shift = float(costs.min())
    ref = R.reference(costs, controls, lam, shift)
    if w_norm is not None:
        w_norm = np.asarray(w_norm)
        w_ref, x, _ = R.weight_errors(costs, lam, w_norm, shift)
        if sum_w is not None:
            allowed = np.maximum((2 * np.abs(x).astype(LD) + E + 2) * LD(R.U) * w_ref, LD(R.TINY) * (E + 1))
            rw = float(np.max(np.abs((w_norm * sum_w).astype(LD) - w_ref) / allowed))
        else:
            wn_ref = (w_ref / ref.S).astype(np.float64)
            allowed = np.maximum((2 * np.abs(x) + E + 2 + K + 1 + ref.xmax + E) * R.U * wn_ref, R.TINY * (E + 1))
            rw = float(np.max(np.abs(w_norm - wn_ref) / allowed))
        report("batch shift", what + " weights", rw)
        assert rw <= 1.0, (what, rw)
        assert abs(math.fsum(w_norm) - 1.0) <= K * R.U, (what, math.fsum(w_norm), K * R.U)
    if sum_w is not None:
        assert sum_w >= 1.0, (what, sum_w)
    check_tail("batch shift", what + " u*", what, ref, E, costs, controls, lam, shift, u_dev, sum_w, stats, sens)
    return ref


def check_handle(group, what, g, lam, u_dev, st, shift=False, sens=True):
    c = g.read_costs()
    return check_update(group, what, c, g.read_controls(), lam, u_dev, st.sum_w, g.read_weights(), st,
                        shift=float(c.min()) if shift else 0.0, sens=sens)


def set_kernel(monkeypatch, kernel):
    if kernel:
        monkeypatch.setenv("CCV_MPPI_KERNEL", kernel)
    else:
        monkeypatch.delenv("CCV_MPPI_KERNEL", raising=False)


def batch_inputs(p, B):
    x0, xr, yr, yaw0 = (np.zeros((B, p.nstate)), np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B))
    paths = [helpers.oracle_path("sinusoid"), helpers.oracle_path("dkan")]
    for b in range(B):
        px, py = paths[b % 2]
        i = 7 * b + 3
        x0[b, 0], x0[b, 1] = px[i], py[i] + 0.05
        x0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
        xr[b], yr[b], yaw = helpers.oracle_window(p, (px, py), x0[b])
        yaw0[b] = yaw[0]
    seeds = np.array([instance_seed(b) for b in range(B)], dtype=np.uint64)
    return x0, xr, yr, yaw0, seeds


def host_controls(p, nominal, seed, it):
    """The batch binding reads no sample controls back: they are rebuilt on the host from the oracle's Philox restatement,
    which is bit-exact with the device (test_noise_bit_exact, test_fused_iteration_matches_oracle_philox)."""
    o = helpers.oracle_for(p)
    o.set_nominal(nominal)
    o.sampling(int(seed), rng="philox", iteration=it)
    return o.get_controls()


def lambdas_for(costs_per_instance, varied):
    """varied: the instances alternate lambda = 1, flat, graded (a leak of one instance's partials into a neighbour's row then
    shows in the flat neighbour); shared: flat for all"""
    out = []
    for b, c in enumerate(costs_per_instance):
        kind = ("one", "flat", "graded")[b % 3] if varied else "flat"
        out.append((kind, 1.0 if kind == "one" else R.regime_lambda(c, kind)))
    return out

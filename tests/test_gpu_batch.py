"""GPU tests of the batch handle (ccv_mppi_batch_*, BatchController): B independent problems in one launch.

Instance b of a batch must compute what a single handle with the same configuration computes for the same inputs and warm
start -- bit for bit where both run the same kernel family, within the cross-kernel tolerances of test_gpu_parity.py
otherwise -- and nothing one instance is given may change another instance's outputs.
"""
import numpy as np
import pytest

import helpers
from batch_support import MODEL_DEFAULTS, families, instance_seed
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController, MPPIError
from oracle import oracle_lib as O

pytestmark = pytest.mark.gpu

TOL_U = 1e-5      # as test_gpu_parity.py
TOL_COST = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def instance_inputs(p, B, salt=0):
    """Distinct inputs per instance: poses along the sinusoid (even b) and dkan (odd b) paths, dt, seeds, warm starts."""
    paths = [helpers.oracle_path("sinusoid"), helpers.oracle_path("dkan")]
    nx = 5 if p.model == "full_body" else 3
    x0, xr, yr = np.zeros((B, nx)), np.zeros((B, p.horizon)), np.zeros((B, p.horizon))
    dt, yaw0 = np.zeros(B), np.zeros(B)
    seeds = np.zeros(B, dtype=np.uint64)
    rng = np.random.default_rng(1234 + salt)
    for b in range(B):
        px, py = paths[b % 2]
        i = (37 * b + 11 * salt + 5) % (len(px) // 2)
        x0[b, 0] = px[i]
        x0[b, 1] = py[i] + 0.05 * ((b % 5) - 2)
        x0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        if nx == 5:
            x0[b, 3], x0[b, 4] = 0.02 * ((b % 3) - 1), -0.01 * (b % 2)
        dt[b] = p.dt * (1.0 + 0.05 * (b % 4))
        _, xr[b], yr[b], yaw = O.calc_ref_path(px, py, x0[b, 0], x0[b, 1], p.v_ref, dt[b], p.resolution, p.horizon)
        yaw0[b] = yaw[0]
        seeds[b] = instance_seed(b, salt)
    lo, hi = np.array(p.u_min), np.array(p.u_max)
    nom = np.clip(0.3 * (hi - lo) / 2 * rng.standard_normal((B, p.horizon - 1, p.udim)) + (hi + lo) / 2, lo, hi)
    return x0, dt, xr, yr, yaw0, seeds, nom


def run_both(p, B, inputs, iters=3):
    """The batch and B single handles from the same warm starts, `iters` consecutive iterations; per iteration the batch's
    (u, stats) and the singles' (u, stats), then the handles."""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat = BatchController(p, B)
    bat.set_nominal(nom)
    singles = [MPPIController(p) for _ in range(B)]
    for b, g in enumerate(singles):
        g.set_nominal(nom[b])
    out = []
    for it in range(iters):
        ub, sb = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        us = [g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), it) for b, g in enumerate(singles)]
        out.append((ub, sb, us))
    return out, bat, singles


def assert_instance_equal(bat, b, g, ub, sb, us_st, exact):
    us, st = us_st
    if exact:
        np.testing.assert_array_equal(ub, us)
        np.testing.assert_array_equal(bat.read_costs(b), g.read_costs())
        np.testing.assert_array_equal(bat.read_weights(b), g.read_weights())
        assert (sb.sum_w, sb.min_cost, sb.max_cost, sb.n_zero_weight, sb.nonfinite) == \
            (st.sum_w, st.min_cost, st.max_cost, st.n_zero_weight, st.nonfinite) or np.isnan(st.sum_w)
    else:
        np.testing.assert_allclose(ub, us, rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(bat.read_costs(b), g.read_costs(), rtol=1e-12)
        np.testing.assert_allclose(bat.read_weights(b), g.read_weights(), rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose([sb.sum_w, sb.min_cost, sb.max_cost], [st.sum_w, st.min_cost, st.max_cost], rtol=1e-8)
        assert sb.n_zero_weight == st.n_zero_weight and sb.nonfinite == st.nonfinite


CASES = [(m, K, H, B) for m in ("diff_drive", "steering_diff_drive")
         for K, H, B in ((1000, 15, 64), (1, 3, 5), (63, 17, 3), (65, 50, 7), (257, 128, 2), (10000, 15, 8))] + \
        [("full_body", 10000, 15, 1), ("full_body", 10000, 15, 4), ("full_body", 130, 9, 3)]


@pytest.mark.parametrize("model,K,H,B", CASES)
def test_batch_equals_single_handles(model, K, H, B):
    p = MODEL_DEFAULTS[model](K, H)
    single_fam, batch_fam = families(model, K, B)
    exact = single_fam == batch_fam
    res, bat, singles = run_both(p, B, instance_inputs(p, B))
    expect = capi.BATCH_KERNEL_FOUR_WAVE if batch_fam == "r4" else capi.BATCH_KERNEL_ONE_WAVE
    assert bat.last_kernel() == expect
    for it, (ub, sb, us) in enumerate(res):
        for b, g in enumerate(singles):
            if it == len(res) - 1:   # (the read-backs are the last iteration's)
                assert_instance_equal(bat, b, g, ub[b], sb[b], us[b], exact)
            elif exact:
                np.testing.assert_array_equal(ub[b], us[b][0])
            else:
                np.testing.assert_allclose(ub[b], us[b][0], rtol=1e-10, atol=1e-13)
    # the states of a few candidates
    for b in (0, B - 1):
        np.testing.assert_allclose(bat.read_candidates(b, 0, min(K, 5), 1), singles[b].read_candidates(0, min(K, 5), 1),
                                   rtol=0 if exact else 1e-13, atol=0 if exact else 1e-13)
    np.testing.assert_array_equal(bat.get_nominal(), res[-1][0])
    bat.close()
    for g in singles:
        g.close()


@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 256, 20, 3), ("steering_diff_drive", 192, 15, 2), ("full_body", 128, 15, 2)])
def test_every_instance_matches_the_oracle(model, K, H, B):
    p = MODEL_DEFAULTS[model](K, H)
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B, salt=3)
    bat = BatchController(p, B)
    bat.set_nominal(nom)
    u_b, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 7)
    for b in range(B):
        o = helpers.oracle_for(p)
        o.set_nominal(nom[b])
        u_o = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=7)
        assert helpers.rel_err(u_b[b], u_o) < TOL_U
        assert np.max(np.abs(bat.read_costs(b) - o.costs()) / o.costs()) < TOL_COST
    bat.close()


def test_instances_are_independent():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 6, 2
    base = instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = [a.copy() for a in base]
    other = instance_inputs(p, B, salt=9)
    x0[j], xr[j], yr[j], yaw0[j], seeds[j] = other[0][j], other[2][j], other[3][j], other[4][j], other[5][j]
    a, b = BatchController(p, B), BatchController(p, B)
    a.set_nominal(base[6])
    b.set_nominal(nom)
    ua, _ = a.iterate(*base[:6], 0)
    ub, _ = b.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert not np.array_equal(ua[j], ub[j])
    for i in range(B):
        if i != j:
            np.testing.assert_array_equal(ua[i], ub[i])
            np.testing.assert_array_equal(a.read_costs(i), b.read_costs(i))


def test_nan_pose_and_underflow_stay_in_their_instance():
    """One instance with a NaN position, one so far from its path that every weight underflows (the set-up of
    test_all_weights_underflow_gives_nan_like_the_reference): each gives what its single handle gives -- the second NaN
    controls with sum_w = 0 and every weight zero -- and every other instance is its single handle's, bit for bit."""
    p = configs.workload("C2").params.with_(num_samples=128, horizon=20, path_weight=1e4)
    B = 4
    path = helpers.oracle_path("sinusoid")
    px, py = path
    x0, dt, xr, yr, yaw0, seeds = np.zeros((B, 3)), np.full(B, p.dt), np.zeros((B, 20)), np.zeros((B, 20)), np.zeros(B), \
        np.arange(1, B + 1, dtype=np.uint64)
    for b, i in enumerate((3, 0, 0, 8)):
        x0[b] = px[i], py[i], np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
    x0[1, :2] = np.nan                  # NaN position (the heading stays finite: the batch keeps its kernel)
    x0[2] = 3.0, 40.0, 0.0              # far from the path: cost >> 745 lambda
    for b in range(B):
        xw, yw, yaw = helpers.oracle_window(p, path, x0[b] if b != 1 else x0[0])
        xr[b], yr[b], yaw0[b] = xw, yw, yaw[0]
    bat = BatchController(p, B)
    ub, sb = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    for b in range(B):
        g = MPPIController(p)
        us, st = g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), 0)
        np.testing.assert_array_equal(ub[b], us)
        np.testing.assert_array_equal(bat.read_costs(b), g.read_costs())
        assert sb[b].n_zero_weight == st.n_zero_weight and sb[b].nonfinite == st.nonfinite
        g.close()
    assert sb[2].sum_w == 0.0 and sb[2].n_zero_weight == 128 and np.all(np.isnan(ub[2])) and sb[2].nonfinite == 1
    for b in (0, 3):
        assert sb[b].sum_w > 0.0 and np.all(np.isfinite(ub[b]))


def test_one_unbounded_heading_sends_the_batch_through_the_plain_kernel():
    p = configs.diff_drive_defaults(256, 20)
    B = 3
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    x0[1, 2] += 1.0e6                    # past the fast sin / cos's range (fast_trig_safe)
    res, bat, singles = run_both(p, B, (x0, dt, xr, yr, yaw0, seeds, nom), iters=1)
    assert bat.last_kernel() == capi.BATCH_KERNEL_PLAIN
    ub, sb, us = res[0]
    for b, g in enumerate(singles):
        np.testing.assert_allclose(ub[b], us[b][0], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(bat.read_costs(b), g.read_costs(), rtol=1e-12)
        o = helpers.oracle_for(p)
        o.set_nominal(nom[b])
        u_o = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=0)
        assert helpers.rel_err(ub[b], u_o) < TOL_U


def test_one_wide_turn_sends_the_batch_through_the_wide_instantiation():
    p = configs.diff_drive_defaults(320, 50)
    B = 3
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    dt[2] = 0.5                          # |w|max dt = 1.0 > pi/4
    path = helpers.oracle_path("sinusoid" if 2 % 2 == 0 else "dkan")
    _, xr[2], yr[2], yaw = O.calc_ref_path(path[0], path[1], x0[2, 0], x0[2, 1], p.v_ref, dt[2], p.resolution, p.horizon)
    yaw0[2] = yaw[0]
    res, bat, singles = run_both(p, B, (x0, dt, xr, yr, yaw0, seeds, nom), iters=2)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE
    ub, sb, us = res[-1]
    for b, g in enumerate(singles):
        assert helpers.rel_err(ub[b], us[b][0]) < 1e-8
        assert np.max(np.abs(bat.read_costs(b) - g.read_costs()) / g.read_costs()) < TOL_COST
        o = helpers.oracle_for(p)
        o.set_nominal(nom[b])
        for it in range(2):
            u_o = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=it)
        assert helpers.rel_err(ub[b], u_o) < TOL_U


def test_blocking_call_equals_enqueue_synchronize_get_nominal():
    p = configs.steering_defaults(1000, 15)
    B = 16
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    a, b = BatchController(p, B), BatchController(p, B)
    a.set_nominal(nom)
    b.set_nominal(nom)
    for it in range(3):
        ua, _ = a.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        b.iterate_enqueue(x0, dt, xr, yr, yaw0, seeds, it)
    b.synchronize()
    np.testing.assert_array_equal(ua, b.get_nominal())
    np.testing.assert_array_equal(a.read_weights(B - 1), b.read_weights(B - 1))
    # the timed path (copies instead of the mailbox) returns the same result and the kernel time
    b.set_nominal(ua)
    a.timing_enable(True)
    u2, st2 = a.iterate(x0, dt, xr, yr, yaw0, seeds, 3)
    u3, _ = b.iterate(x0, dt, xr, yr, yaw0, seeds, 3)
    np.testing.assert_array_equal(u2, u3)
    roll, tot, n = a.timing_read()
    assert n == 1 and 0.0 < roll <= tot and st2[0].rollout_us > 0.0


def test_bad_iteration_arguments_are_refused():
    p = configs.diff_drive_defaults(64, 15)
    B = 2
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    bat = BatchController(p, B)
    with pytest.raises(MPPIError):
        bat.read_costs(0)                # no iteration yet
    dt_nan = dt.copy()
    dt_nan[1] = np.nan
    with pytest.raises(MPPIError) as ei:
        bat.iterate(x0, dt_nan, xr, yr, yaw0, seeds, 0)
    assert ei.value.code == capi.ERR_INVALID_ARG
    import ctypes as C
    d = np.zeros(64)
    s = np.zeros(2, dtype=np.uint64)
    sp = s.ctypes.data_as(C.POINTER(C.c_uint64))
    assert bat.lib.ccv_mppi_batch_iterate(bat._h, None, capi.dptr(d), capi.dptr(d), capi.dptr(d), capi.dptr(d), sp, 0, capi.dptr(d), None) == capi.ERR_INVALID_ARG
    assert bat.lib.ccv_mppi_batch_iterate_enqueue(bat._h, capi.dptr(d), capi.dptr(d), capi.dptr(d), capi.dptr(d), capi.dptr(d), None, 0) == capi.ERR_INVALID_ARG
    bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    for call in (lambda: bat.read_costs(B), lambda: bat.read_costs(0, 60, 5), lambda: bat.read_candidates(0, 0, 2, 64)):
        with pytest.raises(MPPIError):
            call()


def test_batch_create_destroy_returns_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)

    def cycle():
        bat = BatchController(p, B)
        bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        bat.iterate_enqueue(x0, dt, xr, yr, yaw0, seeds, 1)
        bat.read_candidates(B - 1, 0, 4, 1)    # (allocates the read-back scratch)
        assert np.all(np.isfinite(bat.get_nominal()))
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _total = torch.cuda.mem_get_info()
    for _ in range(200):
        cycle()
    torch.cuda.synchronize()
    free1, _total = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 200 create/destroy cycles" % ((free0 - free1) / 2**20)

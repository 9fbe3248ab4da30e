"""GPU tests (-m gpu) of per-instance parameters on batch handles (ccv_mppi_batch_set_params, BatchController with a sequence
of MPPIParams): instance b computes what a single handle created with instance b's parameters computes -- bit for bit where
both run the same kernel family, within the tolerances of test_gpu_batch.py otherwise -- and no parameter of one instance
changes an output bit of another.  The instances differ in every per-instance field: sigma, lambda, v_ref, both bounds and
the six weights.
"""
import numpy as np
import pytest

import ccv_mppi_path_tracker_amd as amd
import helpers
from batch_support import (FAMILY_CODE, MODEL_DEFAULTS, TOL_COST, TOL_U, close_all, families, instance_inputs, path_of,
                           start_poses, stats_tuple, varied)
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController, MPPIError, make_config

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def run_both(seq, inputs, iters=3):
    """The batch with per-instance parameters seq and B single handles made from seq[b], from the same warm starts"""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    B = len(seq)
    bat = BatchController(seq, B)
    bat.set_nominal(nom)
    singles = [MPPIController(q) for q in seq]
    for b, g in enumerate(singles):
        g.set_nominal(nom[b])
    out = []
    for it in range(iters):
        ub, sb = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        us = [g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), it) for b, g in enumerate(singles)]
        out.append((ub, sb, us))
    return out, bat, singles


CASES = [("diff_drive", 1000, 15, 8, False), ("diff_drive", 82048, 15, 2, False),
         ("steering_diff_drive", 1000, 15, 4, False), ("steering_diff_drive", 82048, 15, 2, False),
         ("full_body", 128, 15, 3, False), ("full_body", 130, 9, 3, True), ("full_body", 10000, 15, 4, False)]


@pytest.mark.parametrize("model,K,H,B,roll_off", CASES)
def test_varied_batch_equals_single_handles(model, K, H, B, roll_off):
    """82 048 samples put both the batch and each single handle on the one-wave kernel; full body K = 10 000, B = 4 runs the
    batch on the one-wave kernel and the single handles on the four-wave kernel (tolerances)."""
    p = MODEL_DEFAULTS[model](K, H).with_(roll_off=roll_off)
    single_fam, batch_fam = families(model, K, B)
    exact = single_fam == batch_fam
    seq = varied(p, B)
    res, bat, singles = run_both(seq, instance_inputs(p, B))
    assert bat.last_kernel() == FAMILY_CODE[batch_fam] | capi.BATCH_KERNEL_VARIED
    for it, (ub, sb, us) in enumerate(res):
        for b, g in enumerate(singles):
            if exact:
                np.testing.assert_array_equal(ub[b], us[b][0])
                assert stats_tuple(sb[b]) == stats_tuple(us[b][1])
            else:
                np.testing.assert_allclose(ub[b], us[b][0], rtol=1e-8, atol=1e-11)
                np.testing.assert_allclose([sb[b].sum_w, sb[b].min_cost, sb[b].max_cost],
                                           [us[b][1].sum_w, us[b][1].min_cost, us[b][1].max_cost], rtol=1e-8)
    for b, g in enumerate(singles):   # (the read-backs are the last iteration's)
        if exact:
            np.testing.assert_array_equal(bat.read_costs(b), g.read_costs())
            np.testing.assert_array_equal(bat.read_weights(b), g.read_weights())
        else:
            np.testing.assert_allclose(bat.read_costs(b), g.read_costs(), rtol=1e-12)
            np.testing.assert_allclose(bat.read_weights(b), g.read_weights(), rtol=1e-8, atol=1e-300)
    close_all(bat, singles)


@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 256, 20, 3), ("steering_diff_drive", 192, 15, 2), ("full_body", 128, 15, 2)])
def test_every_instance_matches_the_oracle_with_its_own_parameters(model, K, H, B):
    p = MODEL_DEFAULTS[model](K, H)
    seq = varied(p, B, salt=1)
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B, salt=3)
    bat = BatchController(seq, B)
    bat.set_nominal(nom)
    u_b, _ = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 7)
    for b in range(B):
        o = helpers.oracle_for(seq[b])
        o.set_nominal(nom[b])
        u_o = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=7)
        assert helpers.rel_err(u_b[b], u_o) < TOL_U
        assert np.max(np.abs(bat.read_costs(b) - o.costs()) / o.costs()) < TOL_COST
    bat.close()


def test_copies_of_the_creation_config_are_the_shared_batch_and_null_restores_it():
    p = configs.diff_drive_defaults(1000, 15)
    B = 6
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    shared, per = BatchController(p, B), BatchController(p, B)
    assert per.get_params() == [p] * B
    for h in (shared, per):
        h.set_nominal(nom)
    per.set_params([p] * B)
    for it in range(2):
        ua, sa = shared.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        ub, sb = per.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        np.testing.assert_array_equal(ua, ub)
        assert [stats_tuple(s) for s in sa] == [stats_tuple(s) for s in sb]
    assert shared.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    assert per.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_VARIED
    for b in range(B):
        np.testing.assert_array_equal(shared.read_costs(b), per.read_costs(b))
        np.testing.assert_array_equal(shared.read_weights(b), per.read_weights(b))
    per.set_params(None)
    ua, _ = shared.iterate(x0, dt, xr, yr, yaw0, seeds, 2)
    ub, _ = per.iterate(x0, dt, xr, yr, yaw0, seeds, 2)
    assert per.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    np.testing.assert_array_equal(ua, ub)
    close_all(shared, per)


def test_one_instances_parameters_change_no_bit_of_another():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 6, 2
    seq = varied(p, B)
    seq2 = list(seq)
    seq2[j] = seq[j].with_(control_noise=0.9, lam=7.0, v_ref=0.3, u_min=(-0.4, -1.1), u_max=(0.9, 1.3), path_weight=3.0,
                           v_weight=0.1)
    inputs = instance_inputs(p, B)
    a, b = BatchController(seq, B), BatchController(seq2, B)
    for h in (a, b):
        h.set_nominal(inputs[6])
    for it in range(2):
        ua, _ = a.iterate(*inputs[:6], it)
        ub, _ = b.iterate(*inputs[:6], it)
    assert not np.array_equal(ua[j], ub[j])
    for i in range(B):
        if i != j:
            np.testing.assert_array_equal(ua[i], ub[i])
            np.testing.assert_array_equal(a.read_costs(i), b.read_costs(i))
            np.testing.assert_array_equal(a.read_weights(i), b.read_weights(i))
    close_all(a, b)


def test_clamp_form_is_chosen_per_instance():
    """One instance's bounds out of order in one dimension (the reference's clamp, not the two-instruction one): every
    instance, that one included, is its single handle's bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B = 4
    seq = varied(p, B)
    seq[1] = seq[1].with_(u_min=(0.6, -2.0), u_max=(0.2, 2.0))   # v: u_min > u_max
    res, bat, singles = run_both(seq, instance_inputs(p, B), iters=2)
    ub, sb, us = res[-1]
    for b, g in enumerate(singles):
        np.testing.assert_array_equal(ub[b], us[b][0])
        np.testing.assert_array_equal(bat.read_costs(b), g.read_costs())
    close_all(bat, singles)


def test_one_instance_decides_plain_kernel_and_wide_form():
    p = configs.diff_drive_defaults(256, 20)
    B = 3
    # (a) one instance's turn-rate bounds let headings leave the fast sin / cos range: the whole batch runs the plain kernel
    seq = varied(p, B)
    seq[1] = seq[1].with_(u_min=(-1.2, -1.0e5), u_max=(1.2, 1.0e5))
    res, bat, singles = run_both(seq, instance_inputs(p, B), iters=1)
    assert bat.last_kernel() == capi.BATCH_KERNEL_PLAIN | capi.BATCH_KERNEL_VARIED
    ub, sb, us = res[0]
    for b, g in enumerate(singles):
        np.testing.assert_allclose(ub[b], us[b][0], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(bat.read_costs(b), g.read_costs(), rtol=1e-12)
    close_all(bat, singles)
    # (b) one instance with |w|max dt > pi/4: the wide-turn form
    p = configs.diff_drive_defaults(320, 50)
    seq = varied(p, B)
    seq[2] = seq[2].with_(u_min=(-1.2, -9.0), u_max=(1.2, 9.0))   # 9 * 0.1 > pi/4
    res, bat, singles = run_both(seq, instance_inputs(p, B), iters=2)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE | capi.BATCH_KERNEL_VARIED
    ub, sb, us = res[-1]
    for b, g in enumerate(singles):
        assert helpers.rel_err(ub[b], us[b][0]) < 1e-8
        assert np.max(np.abs(bat.read_costs(b) - g.read_costs()) / g.read_costs()) < TOL_COST
    close_all(bat, singles)


# ---- the device-resident loop ----------------------------------------------------------------------------------------

def test_resident_loop_with_per_instance_v_ref_and_bounds():
    """>= 50 advancing ticks: pose, index, window, trace rows and u* equal (a) the host prologue (calc_ref_path with each
    instance's v_ref, plant_step) driving ccv_mppi_batch_iterate on a batch with the same parameters and (b) B single
    resident handles made from the instances' parameters, bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 6, 56
    seq = varied(p, B)
    assert families(p.model, 1000, B)[0] == families(p.model, 1000, B)[1]
    s0, seeds = start_poses(p, B)
    paths = [path_of(b) for b in range(B)]
    # (a) the host prologue
    host = BatchController(seq, B)
    s, u, ref = s0.copy(), None, []
    for it in range(ticks):
        if it > 0:
            s = np.array([amd.plant_step(p.model, s[b], u[b][0], p.dt) for b in range(B)])
        idx, xr, yr, yaw0 = np.zeros(B, dtype=np.int64), np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B)
        for b in range(B):
            idx[b], xr[b], yr[b], yaw = amd.calc_ref_path(paths[b][0], paths[b][1], s[b, 0], s[b, 1], seq[b].v_ref, p.dt,
                                                          seq[b].resolution, p.horizon)
            yaw0[b] = yaw[0]
        u = host.iterate(s, p.dt, xr, yr, yaw0, seeds, it, want_stats=False)
        ref.append((s.copy(), idx, xr, yr, u.copy()))
    host.close()
    # the resident batch
    bat = BatchController(seq, B)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        if it in (0, 1, 20, ticks - 1):
            st, idx, xr, yr, _, steps = bat.resident_read()
            ws, widx, wxr, wyr, wu = ref[it]
            assert steps == it + 1
            np.testing.assert_array_equal(st, ws)
            np.testing.assert_array_equal(idx, widx)
            np.testing.assert_array_equal(xr, wxr)
            np.testing.assert_array_equal(yr, wyr)
            np.testing.assert_array_equal(bat.get_nominal(), wu)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_VARIED
    for b in range(B):
        tr = bat.resident_read_trace(b)
        np.testing.assert_array_equal(tr[:, :p.nstate], np.array([r[0][b] for r in ref]))
        np.testing.assert_array_equal(tr[:, 5], np.array([r[1][b] for r in ref], dtype=float))
    # (b) single resident handles
    st, idx, xr, yr, yaw0, _ = bat.resident_read()
    ub = bat.get_nominal()
    for b in range(B):
        g = MPPIController(seq[b])
        g.resident_set_path(*paths[b])
        g.resident_set_pose(s0[b])
        for it in range(ticks):
            g.resident_step_enqueue(p.dt, int(seeds[b]), it, advance=it > 0)
        gs, gidx, gxr, gyr, gyaw0, gsteps = g.resident_read()
        assert gsteps == ticks and gidx == idx[b] and gyaw0 == yaw0[b]
        np.testing.assert_array_equal(st[b], gs)
        np.testing.assert_array_equal(xr[b], gxr)
        np.testing.assert_array_equal(yr[b], gyr)
        np.testing.assert_array_equal(ub[b], g.get_nominal())
        g.close()
    bat.close()


def test_refusals_change_nothing():
    p = configs.diff_drive_defaults(1000, 15)
    B = 4
    seq = varied(p, B)
    inputs = instance_inputs(p, B)
    bat, twin = BatchController(seq, B), BatchController(seq, B)
    for h in (bat, twin):
        h.set_nominal(inputs[6])
    lib = capi.load()
    bad = [("model", configs.steering_defaults(1000, 15)), ("num_samples", p.with_(num_samples=512)),
           ("horizon", p.with_(horizon=20)), ("flags", p.with_(roll_off=True))]
    for field, q in bad:
        qs = list(seq)
        qs[2] = q
        cfgs = (capi.Config * B)(*[make_config(x, 0, 0, False, False, x.num_samples) for x in qs])
        assert lib.ccv_mppi_batch_set_params(bat._h, cfgs) == capi.ERR_INVALID_ARG
        msg = lib.ccv_mppi_batch_last_error(bat._h).decode()
        assert "instance 2" in msg and field in msg, msg
    assert bat.get_params() == seq
    ua, _ = bat.iterate(*inputs[:6], 0)
    ub, _ = twin.iterate(*inputs[:6], 0)
    np.testing.assert_array_equal(ua, ub)
    twin.close()
    # resident steps refused before any pose moves: one instance's v_ref gives an unusable stride, one instance's bounds
    # break the angle limit
    s0, seeds = start_poses(p, B)
    bat.resident_set_paths([path_of(b) for b in range(B)])
    bat.resident_set_poses(s0, seeds)
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    bat.resident_step_enqueue(p.dt, 1)
    before = bat.resident_read()
    for q, code in ((seq[1].with_(v_ref=1.0e300), capi.ERR_INVALID_ARG), (seq[1].with_(v_ref=float("nan")), capi.ERR_INVALID_ARG),
                    (seq[1].with_(u_min=(-1.2, -1.0e6), u_max=(1.2, 1.0e6)), capi.ERR_STATE)):
        qs = list(seq)
        qs[1] = q
        bat.set_params(qs)
        with pytest.raises(MPPIError) as e:
            bat.resident_step_enqueue(p.dt, 2)
        assert e.value.code == code
        after = bat.resident_read()
        for k in (0, 1, 2, 3):
            np.testing.assert_array_equal(before[k], after[k])
        assert before[5] == after[5]
    bat.set_params(seq)
    bat.resident_step_enqueue(p.dt, 2)
    assert bat.resident_read()[5] == before[5] + 1
    bat.close()


def test_set_params_flushes_a_pending_resident_update():
    """resident steps, _set_params, resident steps, _set_params(None), resident steps: the same reads as the same sequence
    with a synchronisation after every step"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    seq, seq2 = varied(p, B), varied(p, B, salt=2)
    s0, seeds = start_poses(p, B)

    def run(sync):
        bat = BatchController(seq, B)
        bat.resident_set_paths([path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, seeds)
        reads, it = [], 0

        def steps(n):
            nonlocal it
            for _ in range(n):
                bat.resident_step_enqueue(p.dt, it, advance=it > 0)
                it += 1
                if sync:
                    bat.synchronize()

        steps(3)
        bat.set_params(seq2)
        steps(3)
        reads.append(bat.get_nominal())
        reads.append(bat.resident_read()[0])
        bat.set_params(None)
        steps(3)
        bat.set_params(seq)
        steps(2)
        reads.append(bat.read_costs(B - 1))
        reads.append(bat.get_nominal())
        reads.append(bat.resident_read()[0])
        bat.close()
        return reads

    fused, plain = run(False), run(True)
    for a, b in zip(fused, plain):
        np.testing.assert_array_equal(a, b)


def test_set_params_returns_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    seqs = [varied(p, B, salt=s) for s in range(3)]
    inputs = instance_inputs(p, B)

    def cycle():
        bat = BatchController(p, B)
        for q in seqs:
            bat.set_params(q)
        bat.iterate(*inputs[:6], 0)
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(60):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 60 cycles" % ((free0 - free1) / 2**20)
    # repeated _set_params on one handle does not grow its memory
    bat = BatchController(p, B)
    bat.set_params(seqs[0])
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(300):
        bat.set_params(seqs[i % 3] if i % 5 else None)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 2 * 2**20
    bat.close()


def test_get_params_round_trip():
    p = configs.full_body_defaults(128, 15).with_(steer_off=True)
    B = 3
    bat = BatchController(p, B)
    assert bat.get_params() == [p] * B
    seq = varied(p, B, salt=4)
    bat.set_params(seq)
    assert bat.get_params() == seq
    cfgs = (capi.Config * B)()
    assert capi.load().ccv_mppi_batch_get_params(bat._h, cfgs) == capi.OK
    for b in range(B):
        want = make_config(seq[b], 0, 0, False, False, 128)
        assert bytes(cfgs[b]) == bytes(want)
    bat.set_params(None)
    assert bat.get_params() == [p] * B
    bat.close()

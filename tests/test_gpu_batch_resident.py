"""GPU tests (-m gpu) of the batch handles' device-resident closed loop (ccv_mppi_batch_resident_*,
BatchController.resident_*): get_CurrentIndex() + calc_RefPath() + the closed-loop plant of B instances on the device.

Checkers: the same batch driven by the host prologue (ccv_mppi_calc_ref_path / ccv_mppi_plant_step per instance, then
BatchController.iterate) -- index, window, pose and u* bit for bit, yaw_ref[0] (device atan2) to 4 ulp -- and B single
resident handles: bit for bit where both run the same kernel family, to the cross-kernel tolerances of test_gpu_batch.py
otherwise.  Each instance runs on its own path (even instances the sinusoid, odd ones dkan), pose and seed.
"""
import numpy as np
import pytest

import ccv_mppi_path_tracker_amd as amd
from batch_support import MODEL_DEFAULTS, families, instance_seed, path_of
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController, MPPIError
from resident_loops import host_batch_loop, resident_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def start_poses(p, B, salt=0):
    """A pose near its path per instance, and a seed."""
    s = np.zeros((B, p.nstate))
    seeds = np.zeros(B, dtype=np.uint64)
    for b in range(B):
        px, py = path_of(b)
        i = (37 * b + 11 * salt + 5) % (len(px) // 2)
        s[b, 0] = px[i]
        s[b, 1] = py[i] + 0.05 * ((b % 5) - 2)
        s[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        if p.nstate == 5:
            s[b, 3], s[b, 4] = 0.02 * ((b % 3) - 1), -0.01 * (b % 2)
        seeds[b] = instance_seed(b, salt)
    return s, seeds


def assert_ulp(a, b, n=4):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.abs(a - b) <= n * np.spacing(np.abs(b))), (a, b)


@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 1000, 15, 8), ("diff_drive", 63, 17, 3),
                                         ("steering_diff_drive", 1000, 15, 8), ("steering_diff_drive", 63, 17, 3)])
def test_resident_batch_is_the_host_prologue_batch_bit_for_bit(model, K, H, B):
    p = MODEL_DEFAULTS[model](K, H)
    s0, seeds = start_poses(p, B)
    ticks = 25
    ref = host_batch_loop(p, B, K, s0, seeds, ticks)
    bat = resident_batch(p, B, K, s0, seeds)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        if it in (0, 1, 7, ticks - 1):   # (reading synchronises; the ticks in between run back to back)
            st, idx, xr, yr, yaw0, steps = bat.resident_read()
            s, widx, wxr, wyr, wyaw0, u = ref[it]
            assert steps == it + 1
            np.testing.assert_array_equal(idx, widx)
            np.testing.assert_array_equal(st, s)
            np.testing.assert_array_equal(xr, wxr)
            np.testing.assert_array_equal(yr, wyr)
            assert_ulp(yaw0, wyaw0)
            np.testing.assert_array_equal(bat.get_nominal(), u)
    for b in range(B):
        tr = bat.resident_read_trace(b)
        assert tr.shape == (ticks, 6)
        np.testing.assert_array_equal(tr[:, :p.nstate], np.array([r[0][b] for r in ref]))
        np.testing.assert_array_equal(tr[:, 5], np.array([r[1][b] for r in ref], dtype=float))
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    bat.close()


@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 1000, 15, 4), ("steering_diff_drive", 257, 20, 3),
                                         ("diff_drive", 1000, 15, 96)])
def test_resident_batch_equals_single_resident_handles(model, K, H, B):
    """B = 96 at K = 1 000 puts the batch on the one-wave kernel (96 * 16 workgroups > 5 per CU) while each single handle
    keeps the four-wave kernel: the cross-kernel tolerances apply there."""
    p = MODEL_DEFAULTS[model](K, H)
    single_fam, batch_fam = families(model, K, B)
    exact = single_fam == batch_fam
    s0, seeds = start_poses(p, B, salt=1)
    ticks = 8 if exact else 4
    bat = resident_batch(p, B, K, s0, seeds)
    singles = []
    for b in range(B):
        g = MPPIController(p, num_samples=K)
        g.resident_set_path(*path_of(b))
        g.resident_set_pose(s0[b])
        singles.append(g)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        for b, g in enumerate(singles):
            g.resident_step_enqueue(p.dt, int(seeds[b]), it, advance=it > 0)
    expect = capi.BATCH_KERNEL_FOUR_WAVE if batch_fam == "r4" else capi.BATCH_KERNEL_ONE_WAVE
    assert bat.last_kernel() == expect
    st, idx, xr, yr, yaw0, steps = bat.resident_read()
    ub = bat.get_nominal()
    assert steps == ticks
    for b, g in enumerate(singles):
        gs, gidx, gxr, gyr, gyaw0, gsteps = g.resident_read()
        assert gsteps == ticks and idx[b] == gidx
        if exact:
            np.testing.assert_array_equal(st[b], gs)
            np.testing.assert_array_equal(xr[b], gxr)
            np.testing.assert_array_equal(yr[b], gyr)
            assert yaw0[b] == gyaw0
            np.testing.assert_array_equal(ub[b], g.get_nominal())
        else:
            np.testing.assert_allclose(st[b], gs, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(xr[b], gxr, rtol=0, atol=0)
            np.testing.assert_allclose(ub[b], g.get_nominal(), rtol=1e-8, atol=1e-11)
        g.close()
    bat.close()


def test_resident_batch_full_body_within_tolerance():
    """fb:408 reads yaw_ref[0] (device atan2 vs libm: last-place differences): the tolerances of
    test_resident_loop_full_body_within_tolerance."""
    p = configs.workload("C4", num_samples=1024).params
    B, K, ticks = 3, 1024, 12
    s0, seeds = start_poses(p, B)
    ref = host_batch_loop(p, B, K, s0, seeds, ticks)
    bat = resident_batch(p, B, K, s0, seeds)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
    st, idx, xr, yr, yaw0, steps = bat.resident_read()
    s, widx, wxr, wyr, wyaw0, u = ref[-1]
    assert steps == ticks
    np.testing.assert_array_equal(idx, widx)
    np.testing.assert_allclose(st, s, rtol=0, atol=1e-9)
    np.testing.assert_allclose(bat.get_nominal(), u, rtol=1e-7, atol=1e-9)
    bat.close()


def test_resident_batch_instances_are_independent():
    p = configs.diff_drive_defaults(1000, 15)
    B, j, ticks = 6, 3, 20
    s0, seeds = start_poses(p, B)
    paths = [path_of(b) for b in range(B)]
    s1, seeds1, paths1 = s0.copy(), seeds.copy(), list(paths)
    px, py = paths[j]
    paths1[j] = (px * 1.01 + 0.3, py - 0.2)
    s1[j, :3] = px[40] + 0.3, py[40] - 0.15, 0.4
    seeds1[j] = 12345
    a = resident_batch(p, B, 1000, s0, seeds, paths)
    b = resident_batch(p, B, 1000, s1, seeds1, paths1)
    for it in range(ticks):
        a.resident_step_enqueue(p.dt, it, advance=it > 0)
        b.resident_step_enqueue(p.dt, it, advance=it > 0)
    ra, rb = a.resident_read(), b.resident_read()
    ua, ub = a.get_nominal(), b.get_nominal()
    assert not np.array_equal(ra[0][j], rb[0][j]) and not np.array_equal(ua[j], ub[j])
    others = [i for i in range(B) if i != j]
    for k in range(4):   # pose, index, x_ref, y_ref
        np.testing.assert_array_equal(ra[k][others], rb[k][others])
    np.testing.assert_array_equal(ua[others], ub[others])
    a.close()
    b.close()


def test_resident_batch_gate_ties_and_path_end_per_instance():
    """In one batch: an instance > 100 m from its path (index 0), one past the end of its path (the window repeats the final
    pose), one at equal distance from two poses (the first wins), and an ordinary one -- each as calc_ref_path gives it."""
    p = configs.diff_drive_defaults(256, 30)
    t = np.arange(700) * 0.1
    loop = (np.concatenate([t, t[::-1]]), np.zeros(2 * len(t)))      # passes every point twice
    straight = amd.make_path("straight")
    sinus = path_of(0)
    paths = [sinus, straight, loop, path_of(1)]
    poses = np.array([[sinus[0][0] + 150.0, sinus[1][0] + 80.0, 0.0],
                      [straight[0][-3], 0.0, 0.0],
                      [3.0, 0.2, 0.0],
                      [path_of(1)[0][50], path_of(1)[1][50] + 0.1, 0.3]])
    bat = BatchController(p, 4)
    bat.resident_set_paths(paths, [0.1, 0.1, 0.1, p.resolution])
    bat.resident_set_poses(poses, [1, 2, 3, 4])
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    st, idx, xr, yr, yaw0, _ = bat.resident_read()
    np.testing.assert_array_equal(st, poses)
    for b, res in enumerate((0.1, 0.1, 0.1, p.resolution)):
        want_idx, wxr, wyr, _ = amd.calc_ref_path(paths[b][0], paths[b][1], poses[b, 0], poses[b, 1], p.v_ref, p.dt, res,
                                                  p.horizon)
        assert idx[b] == want_idx
        np.testing.assert_array_equal(xr[b], wxr)
        np.testing.assert_array_equal(yr[b], wyr)
    assert idx[0] == 0
    assert xr[1][-1] == straight[0][-1] and yr[1][-1] == straight[1][-1] and xr[1][-2] == straight[0][-1]
    assert idx[2] < 700                  # the first of the two equal distances


def test_resident_batch_refusals_move_nothing(monkeypatch):
    p = configs.steering_defaults(256, 20)
    B = 3
    s0, seeds = start_poses(p, B)
    bat = BatchController(p, B)
    with pytest.raises(MPPIError) as e:
        bat.resident_step_enqueue(p.dt, 0)                               # no paths
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(MPPIError) as e:
        bat.resident_set_poses(s0, seeds)                               # poses before paths
    assert e.value.code == capi.ERR_STATE
    bat.resident_set_paths([path_of(b) for b in range(B)])
    with pytest.raises(MPPIError) as e:
        bat.resident_step_enqueue(p.dt, 0)                               # no poses
    assert e.value.code == capi.ERR_STATE
    bat.resident_set_poses(s0, seeds)
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    bat.resident_step_enqueue(p.dt, 1)
    before = bat.resident_read()

    def refused(code, call):
        with pytest.raises(MPPIError) as e:
            call()
        assert e.value.code == code
        after = bat.resident_read()
        np.testing.assert_array_equal(before[0], after[0])
        np.testing.assert_array_equal(before[1], after[1])
        assert before[5] == after[5]

    for dt in (np.nan, -0.1, np.inf):
        refused(capi.ERR_INVALID_ARG, lambda: bat.resident_step_enqueue(dt, 2))
    bat.resident_set_paths([path_of(b) for b in range(B)], [p.resolution, 1e-300, p.resolution])   # one unusable stride
    refused(capi.ERR_INVALID_ARG, lambda: bat.resident_step_enqueue(p.dt, 2))
    bat.resident_set_paths([path_of(b) for b in range(B)])
    # an absurd steering ANGLE in one instance's warm start is added to its heading before sin / cos
    u = bat.get_nominal()
    huge = u.copy()
    huge[1, 0, 2] = 5.0e6
    bat.set_nominal(huge)
    refused(capi.ERR_STATE, lambda: bat.resident_step_enqueue(p.dt, 2))
    bat.set_nominal(u)
    bat.resident_step_enqueue(p.dt, 2)
    # one instance with an unbounded yaw: refused before anything moves
    s_bad = s0.copy()
    s_bad[2, 2] = 2.0e5
    bat.resident_set_poses(s_bad, seeds)
    before = bat.resident_read()
    refused(capi.ERR_STATE, lambda: bat.resident_step_enqueue(p.dt, 0, advance=False))
    bat.close()
    # the plain kernel (CCV_MPPI_KERNEL=v1) has no resident form
    monkeypatch.setenv("CCV_MPPI_KERNEL", "v1")
    v1 = BatchController(p, B)
    v1.resident_set_paths([path_of(b) for b in range(B)])
    v1.resident_set_poses(s0, seeds)
    with pytest.raises(MPPIError) as e:
        v1.resident_step_enqueue(p.dt, 0, advance=False)
    assert e.value.code == capi.ERR_STATE
    assert v1.resident_read()[5] == 0
    v1.close()


def test_resident_batch_refuses_a_nan_command_in_the_warm_start():
    """As the single handle's test: a NaN in row 0 of one instance's warm start, finite values everywhere else, is refused
    with the state error before any pose moves."""
    p = configs.diff_drive_defaults(256, 20)
    B = 3
    s0, seeds = start_poses(p, B)
    bat = BatchController(p, B)
    bat.resident_set_paths([path_of(b) for b in range(B)])
    bat.resident_set_poses(s0, seeds)
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    u = np.full((B, p.horizon - 1, p.udim), 0.1)
    u[1, 0, 1] = np.nan
    bat.set_nominal(u)
    before = bat.resident_read()
    with pytest.raises(MPPIError) as e:
        bat.resident_step_enqueue(p.dt, 1)
    assert e.value.code == capi.ERR_STATE
    after = bat.resident_read()
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    assert before[5] == after[5] == 1
    bat.set_nominal(np.full((B, p.horizon - 1, p.udim), 0.1))
    bat.resident_step_enqueue(p.dt, 1)
    assert np.all(np.isfinite(bat.resident_read()[0]))
    bat.close()


def test_resident_batch_mixing_and_flush_points():
    """resident steps -> get_nominal -> iterate (host records) -> resident steps -> set_nominal -> resident steps ->
    read_costs: at every read the u* (and pose) of the same sequence with synchronize() after every step, where no update is
    ever fused with a prologue."""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    s0, seeds = start_poses(p, B)

    def run(sync):
        bat = resident_batch(p, B, 1000, s0, seeds)
        reads, it = [], 0

        def steps(n):
            nonlocal it
            for _ in range(n):
                bat.resident_step_enqueue(p.dt, it, advance=it > 0)
                it += 1
                if sync:
                    bat.synchronize()

        steps(3)
        reads.append(bat.get_nominal())
        st, idx, xr, yr, yaw0, _ = bat.resident_read()
        u, _ = bat.iterate(st, p.dt, xr, yr, yaw0, seeds + np.uint64(7), 100)
        reads.append(u)
        steps(3)
        reads.append(bat.resident_read()[0])
        reads.append(bat.get_nominal())
        bat.set_nominal(0.5 * reads[-1])
        steps(3)
        reads.append(bat.read_costs(B - 1))
        reads.append(bat.get_nominal())
        reads.append(bat.resident_read()[0])
        bat.close()
        return reads

    fused, plain = run(False), run(True)
    for a, b in zip(fused, plain):
        np.testing.assert_array_equal(a, b)


def test_resident_batch_create_destroy_returns_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    s0, seeds = start_poses(p, B)
    paths = [path_of(b) for b in range(B)]

    def cycle():
        bat = resident_batch(p, B, 1000, s0, seeds, paths)
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        bat.resident_step_enqueue(p.dt, 1)
        bat.close()   # (with the second tick's update still pending)

    for _ in range(3):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _total = torch.cuda.mem_get_info()
    for _ in range(100):
        cycle()
    torch.cuda.synchronize()
    free1, _total = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 100 create/destroy cycles" % ((free0 - free1) / 2**20)

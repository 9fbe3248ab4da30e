"""GPU tests (-m gpu) of the device-resident closed loop (include/ccv_mppi.h, "device-resident closed loop"):
get_CurrentIndex() + calc_RefPath() (dd:126-181) and the closed-loop plant on the device.

Checker: the host prologue (ccv_mppi_calc_ref_path / ccv_mppi_plant_step, themselves checked against the oracle in
tests/test_host_prologue.py) driving the ordinary ccv_mppi_iterate path.  Everything integer or copied (index, x_ref,
y_ref) and everything computed with specified arithmetic (pose, window coefficients -> u*) must be bit-identical;
yaw_ref[0] comes from the device atan2 and is compared to 4 ulp (it only enters the full-body yaw cost, fb:408).
"""
import numpy as np
import pytest

import helpers
import ccv_mppi_path_tracker_amd as amd
from ccv_mppi_path_tracker_amd import capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController, MPPIError
from resident_loops import host_loop

pytestmark = pytest.mark.gpu

WORKLOADS = {"diff_drive": "C2", "steering_diff_drive": "C3", "full_body": "C4"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def start(p, px, py, lateral=0.05):
    s = np.zeros(p.nstate)
    s[0], s[1], s[2] = px[0], py[0] + lateral, 0.02
    return s


@pytest.mark.parametrize("model", ["diff_drive", "steering_diff_drive"])
def test_resident_loop_is_the_host_loop_bit_for_bit(model):
    w = configs.workload(WORKLOADS[model], num_samples=1024)
    p = w.params
    px, py = amd.make_path(w.path)
    s0 = start(p, px, py)
    ticks, seed = 25, 77
    poses, wins, us = host_loop(p, px, py, s0, ticks, seed, 1024)
    g = MPPIController(p, num_samples=1024)
    g.resident_set_path(px, py)
    g.resident_set_pose(s0)
    for it in range(ticks):
        g.resident_step_enqueue(p.dt, seed, it, advance=it > 0)
        if it in (0, 1, 7, ticks - 1):   # (reading synchronises; the ticks in between run back to back)
            st, idx, xr, yr, yaw0, steps = g.resident_read()
            assert steps == it + 1
            assert idx == wins[it][0]
            np.testing.assert_array_equal(st, poses[it])
            np.testing.assert_array_equal(xr, wins[it][1])
            np.testing.assert_array_equal(yr, wins[it][2])
            assert abs(yaw0 - wins[it][3]) <= 4 * np.spacing(abs(wins[it][3]))
            np.testing.assert_array_equal(g.get_nominal(), us[it])
    tr = g.resident_read_trace()
    assert tr.shape == (ticks, 6)
    np.testing.assert_array_equal(tr[:, :3], np.array(poses))
    np.testing.assert_array_equal(tr[:, 5], np.array([wn[0] for wn in wins], dtype=float))
    assert tr[-1, 0] > tr[0, 0] + 0.2   # the loop drove along the path


def test_resident_loop_full_body_within_tolerance():
    """fb:408 reads yaw_ref[0] (device atan2 vs libm: last-place differences), so the loop is compared to tolerance."""
    w = configs.workload("C4", num_samples=1024)
    p = w.params
    px, py = amd.make_path(w.path)
    s0 = start(p, px, py)
    ticks, seed = 12, 5
    poses, wins, us = host_loop(p, px, py, s0, ticks, seed, 1024)
    g = MPPIController(p, num_samples=1024)
    g.resident_set_path(px, py)
    g.resident_set_pose(s0)
    for it in range(ticks):
        g.resident_step_enqueue(p.dt, seed, it, advance=it > 0)
    st, idx, xr, yr, yaw0, steps = g.resident_read()
    assert steps == ticks and idx == wins[-1][0]
    np.testing.assert_allclose(st, poses[-1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(g.get_nominal(), us[-1], rtol=1e-7, atol=1e-9)


def test_resident_index_gate_ties_and_path_end():
    """get_CurrentIndex(): first of equal distances, index 0 when nothing is inside the 100 m gate; calc_RefPath():
    the final pose repeats past the end of the path (dd:169-172)."""
    p = configs.diff_drive_defaults(256, 30)
    # a path that passes the same point twice (equal distances), longer than one scan stride of the kernel
    t = np.arange(700) * 0.1
    px = np.concatenate([t, t[::-1]])
    py = np.zeros_like(px)
    g = MPPIController(p)
    g.resident_set_path(px, py, 0.1)
    for pose in ([3.0, 0.2, 0.0], [69.9, -0.1, 0.0], [500.0, 0.0, 0.0], [-20.0, 5.0, 1.0], [35.0, 0.0, 0.0]):
        g.resident_set_pose(pose)
        g.resident_step_enqueue(p.dt, 1, 0, advance=False)
        st, idx, xr, yr, yaw0, _ = g.resident_read()
        want_idx, wxr, wyr, wyaw = amd.calc_ref_path(px, py, pose[0], pose[1], p.v_ref, p.dt, 0.1, p.horizon)
        assert idx == want_idx
        np.testing.assert_array_equal(xr, wxr)
        np.testing.assert_array_equal(yr, wyr)
        np.testing.assert_array_equal(st, pose)
    # near the end of a short path the window runs past it
    px2, py2 = amd.make_path("straight")
    g.resident_set_path(px2, py2, 0.1)
    g.resident_set_pose([px2[-3], 0.0, 0.0])
    g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    _, idx, xr, yr, _, _ = g.resident_read()
    want_idx, wxr, wyr, _ = amd.calc_ref_path(px2, py2, px2[-3], 0.0, p.v_ref, p.dt, 0.1, p.horizon)
    assert idx == want_idx == len(px2) - 3
    np.testing.assert_array_equal(xr, wxr)
    assert xr[-1] == px2[-1] and xr[5] == px2[-1]


def test_resident_partials_step_matches_plain_step():
    """K-sharded form: [sum w, sum w*u] left in a device buffer, applied afterwards -- same u*, same poses."""
    import torch
    w = configs.workload("C2", num_samples=2048)
    p = w.params
    px, py = amd.make_path(w.path)
    s0 = start(p, px, py)
    a, b = MPPIController(p), MPPIController(p)
    vec = torch.zeros(b.partials_size(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for g in (a, b):
        g.resident_set_path(px, py)
        g.resident_set_pose(s0)
    for it in range(6):
        a.resident_step_enqueue(p.dt, 9, it, advance=it > 0)
        b.resident_step_partials_enqueue(p.dt, 9, it, it > 0, vec.data_ptr())
        b.apply_partials_enqueue(vec.data_ptr())
    np.testing.assert_array_equal(a.resident_read()[0], b.resident_read()[0])
    np.testing.assert_allclose(a.get_nominal(), b.get_nominal(), rtol=1e-12, atol=0)


def test_resident_sharded_driver_two_shards_one_device():
    """ShardedMPPI.iterate_resident over two shards of K held by two handles on this device (the all-reduce done by hand):
    same poses and u* as one handle with all K, to summation order."""
    import torch
    from ccv_mppi_path_tracker_amd import sharded
    w = configs.workload("C2", num_samples=2048)
    p = w.params
    px, py = amd.make_path(w.path)
    s0 = start(p, px, py)
    whole = MPPIController(p)
    whole.resident_set_path(px, py)
    whole.resident_set_pose(s0)
    # a dedicated torch stream, as bench.py does: DevicePartials puts its handle on torch's current stream, so the handles'
    # kernels and the stand-in for the all-reduce below are ordered (the null stream would mean "the handle's own stream")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        halves = [sharded.DevicePartials(MPPIController(p, num_samples=1024, sample_offset=o)) for o in (0, 1024)]
        for h in halves:
            h.resident_setup(px, py, s0)
        for it in range(8):
            whole.resident_step_enqueue(p.dt, 3, it, advance=it > 0)
            parts = [h.local_partials_resident(p.dt, 3, it, it > 0) for h in halves]
            total = parts[0] + parts[1]
            for h in halves:
                h.apply(total)
                h.ctl.synchronize()   # (total is a temporary: apply now instead of deferring)
    want = whole.resident_read()[0]
    for h in halves:
        np.testing.assert_allclose(h.ctl.resident_read()[0], want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h.ctl.get_nominal(), whole.get_nominal(), rtol=1e-9, atol=1e-12)


def test_resident_loop_with_direct_exchange_single_rank():
    """The resident loop through ExchangeBackend (world = 1: the box is this device's own) follows the plain resident loop."""
    from ccv_mppi_path_tracker_amd import sharded
    w = configs.workload("C2", num_samples=2048)
    p = w.params
    px, py = amd.make_path(w.path)
    s0 = start(p, px, py)
    a, b = MPPIController(p), MPPIController(p)
    a.resident_set_path(px, py)
    a.resident_set_pose(s0)
    xb = sharded.ExchangeBackend(b)
    assert xb.ok
    xb.resident_setup(px, py, s0)
    drv = sharded.ShardedMPPI(xb)
    for it in range(8):
        a.resident_step_enqueue(p.dt, 4, it, advance=it > 0)
        drv.iterate_resident(p.dt, 4, it, advance=it > 0)
    np.testing.assert_array_equal(a.resident_read()[0], b.resident_read()[0])
    np.testing.assert_array_equal(a.get_nominal(), b.get_nominal())


def test_resident_errors():
    p = configs.diff_drive_defaults(256, 30)
    g = MPPIController(p)
    with pytest.raises(MPPIError):
        g.resident_step_enqueue(p.dt, 1, 0)          # no path
    with pytest.raises(MPPIError):
        g.resident_set_pose([0, 0, 0])               # no path yet
    px, py = amd.make_path("straight")
    with pytest.raises(MPPIError):
        g.resident_set_path(px, py, 0.0)             # resolution
    g.resident_set_path(px, py, 0.1)
    with pytest.raises(MPPIError):
        g.resident_step_enqueue(p.dt, 1, 0)          # no pose
    g.resident_set_pose([0, 0, 0])
    with pytest.raises(MPPIError):
        g.resident_step_enqueue(float("nan"), 1, 0)
    g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    assert np.all(np.isfinite(g.get_nominal()))


def test_resident_rejects_bad_dt_before_moving_the_pose():
    """dt is the stride of the window index (dd:160-163): negative and infinite periods are refused like NaN, on the
    device path and in ccv_mppi_calc_ref_path alike, and a refused step leaves the pose and the step counter alone
    (dt = 0 is defined -- stride 0 -- and admitted by both: test_resident_zero_dt_matches_host_prologue)."""
    p = configs.diff_drive_defaults(256, 30)
    px, py = amd.make_path("sinusoid")
    g = MPPIController(p)
    g.resident_set_path(px, py, 0.1)
    g.resident_set_pose([0.3, 0.1, 0.2])
    g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    before = g.resident_read()
    for bad in (-0.1, float("inf"), float("-inf"), float("nan"), 1e300):
        with pytest.raises(MPPIError) as e:
            g.resident_step_enqueue(bad, 1, 1, advance=True)
        assert e.value.code == capi.ERR_INVALID_ARG
        with pytest.raises(MPPIError):
            amd.calc_ref_path(px, py, 0.3, 0.1, p.v_ref, bad, p.resolution, p.horizon)
    after = g.resident_read()
    np.testing.assert_array_equal(before[0], after[0])
    assert before[5] == after[5] == 1
    with pytest.raises(MPPIError):
        amd.calc_ref_path(px, py, 0.3, 0.1, -1.0, 0.1, p.resolution, p.horizon)   # negative stride


@pytest.mark.parametrize("model", ["diff_drive", "full_body"])
def test_resident_loop_runs_past_the_angle_limit(model):
    """Round 1 bounded |yaw| of the resident pose by accumulation and refused every step once the bound passed 1e5 rad
    (about 5e5 ticks at the C2 limits).  Now the plant takes an angle modulo 2 pi once it leaves +-1e4 rad, on the device
    and in ccv_mppi_plant_step alike: a loop started just below that limit and turning hard crosses it, keeps running, and
    stays the host loop bit for bit (diff drive); 3000 more ticks never refuse."""
    w = configs.workload(WORKLOADS[model], num_samples=512, horizon=20)
    p = w.params.with_(yaw_weight=0.0)   # (fb:408: 2 * (1e4)^2 would underflow every weight -- SURVEY Q15 / Q4)
    px, py = amd.make_path("straight")
    s0 = np.zeros(p.nstate)
    s0[:3] = 1.0, 0.2, 1.0e4 - 0.35
    turn = np.zeros((p.horizon - 1, p.udim))
    turn[:, 0], turn[:, 1] = 0.5, p.u_max[1]      # warm start: turn left as hard as allowed
    ticks, seed = 12, 5
    g = MPPIController(p)
    g.resident_set_path(px, py)
    g.resident_set_pose(s0)
    g.set_nominal(turn)
    h = MPPIController(p)
    h.set_nominal(turn)
    s, u, crossed = s0.copy(), None, False
    for it in range(ticks):
        g.resident_step_enqueue(p.dt, seed, it, advance=it > 0)
        if it > 0:
            s = amd.plant_step(p.model, s, u[0], p.dt)
        crossed = crossed or abs(s[2]) < 10.0
        idx, xr, yr, yaw = amd.calc_ref_path(px, py, s[0], s[1], p.v_ref, p.dt, p.resolution, p.horizon)
        u = h.iterate(s, p.dt, xr, yr, yaw[0], seed, it, want_stats=False)
        if model == "diff_drive":
            np.testing.assert_array_equal(g.resident_read()[0], s)
            np.testing.assert_array_equal(g.get_nominal(), u)
        else:
            np.testing.assert_allclose(g.resident_read()[0], s, rtol=0, atol=1e-9)
    assert crossed, "the loop never crossed the re-basing limit"
    for it in range(ticks, ticks + 3000):
        g.resident_step_enqueue(p.dt, seed, it, advance=True)
    st = g.resident_read()[0]
    assert np.all(np.isfinite(st)) and abs(st[2]) <= 1.0e4 + 1.0


def test_resident_refuses_unbounded_angles_and_commands():
    p = configs.diff_drive_defaults(256, 30)
    px, py = amd.make_path("straight")
    g = MPPIController(p)
    g.resident_set_path(px, py)
    g.resident_set_pose([0.0, 0.0, 2.0e5])                      # outside the sin/cos range from the start
    with pytest.raises(MPPIError) as e:
        g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    assert e.value.code == capi.ERR_STATE
    g.resident_set_pose([0.0, 0.0, 9.0e4])                      # inside: runs, and the first advance re-bases it
    g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    g.resident_step_enqueue(p.dt, 1, 1, advance=True)
    assert abs(g.resident_read()[0][2]) <= np.pi + 1.0
    # an absurd yaw RATE in a caller's warm start is harmless: the plant re-bases the yaw it produces
    huge = np.zeros((p.horizon - 1, p.udim))
    huge[0, 1] = 5.0e6
    g.set_nominal(huge)
    g.resident_step_enqueue(p.dt, 1, 2, advance=True)
    assert abs(g.resident_read()[0][2]) <= np.pi and np.all(np.isfinite(g.get_nominal()))
    # an absurd steering ANGLE is added to the heading before its sin / cos: part of the bound, refused before the pose moves
    ps = configs.steering_defaults(256, 30)
    gs = MPPIController(ps)
    gs.resident_set_path(px, py)
    gs.resident_set_pose([0.0, 0.0, 0.1])
    gs.resident_step_enqueue(ps.dt, 1, 0, advance=False)
    huge = np.zeros((ps.horizon - 1, ps.udim))
    huge[0, 2] = 5.0e6
    gs.set_nominal(huge)
    before = gs.resident_read()
    with pytest.raises(MPPIError) as e:
        gs.resident_step_enqueue(ps.dt, 1, 1, advance=True)
    assert e.value.code == capi.ERR_STATE
    after = gs.resident_read()
    np.testing.assert_array_equal(before[0], after[0])
    assert before[5] == after[5]
    gs.set_nominal(np.zeros((ps.horizon - 1, ps.udim)))
    gs.resident_step_enqueue(ps.dt, 1, 1, advance=True)
    assert np.all(np.isfinite(gs.get_nominal()))


def test_resident_refuses_a_nan_command_in_the_warm_start():
    """A NaN in row 0 of a caller's warm start is the command u*[0] of the next advancing step: refused with the state error
    before the pose moves, however many finite values of the same control dimension follow it (the bound on |u*| keeps the
    NaN)."""
    p = configs.diff_drive_defaults(256, 30)
    px, py = amd.make_path("straight")
    g = MPPIController(p)
    g.resident_set_path(px, py)
    g.resident_set_pose([0.3, 0.1, 0.2])
    g.resident_step_enqueue(p.dt, 1, 0, advance=False)
    u = np.full((p.horizon - 1, p.udim), 0.1)
    u[0, 1] = np.nan
    g.set_nominal(u)
    before = g.resident_read()
    with pytest.raises(MPPIError) as e:
        g.resident_step_enqueue(p.dt, 1, 1, advance=True)
    assert e.value.code == capi.ERR_STATE
    after = g.resident_read()
    np.testing.assert_array_equal(before[0], after[0])
    assert before[5] == after[5] == 1
    g.set_nominal(np.full((p.horizon - 1, p.udim), 0.1))
    g.resident_step_enqueue(p.dt, 1, 1, advance=True)
    assert np.all(np.isfinite(g.resident_read()[0]))


def test_resident_closed_loop_at_full_c2_size():
    """The device-resident closed loop at the headline size (C2: K = 65 536, T = 50, sinusoid), as bench.py's closed_loop leg
    runs it: 512 ticks back to back with no host data, the pose fed back every tick.  The robot must track the course
    (RMS distance to the nearest path pose < 0.1 m -- the reference's own notion of "works", calc_e_rmse.py:30-49) and
    two runs must end with identical bits everywhere (trace, warm start): the loop has no atomics and no run-to-run freedom."""
    w = configs.workload("C2")
    p = w.params
    ticks = 512
    need = (ticks + 8) * max(abs(p.u_max[0]), abs(p.u_min[0])) * p.dt + 2.0 * p.horizon * p.v_ref * p.dt
    px, py = amd.make_path(w.path, p.resolution, length=need)
    s0 = np.zeros(p.nstate)
    s0[0], s0[1] = px[0], py[0]
    runs = []
    for rep in range(2):
        g = MPPIController(p)
        g.resident_set_path(px, py)
        g.resident_set_pose(s0)
        for i in range(ticks):
            g.resident_step_enqueue(p.dt, 42, i, advance=i > 0)
        g.synchronize()
        runs.append((g.resident_read_trace(max_rows=ticks), g.get_nominal(), g.resident_read()))
        g.close()
    tr = runs[0][0]
    assert tr.shape == (ticks, 6) and np.all(np.isfinite(tr))
    d = np.hypot(px[None, :] - tr[:, 0:1], py[None, :] - tr[:, 1:2]).min(axis=1)
    assert np.sqrt(np.mean(d * d)) < 0.1 and d.max() < 0.3
    assert np.hypot(np.diff(tr[:, 0]), np.diff(tr[:, 1])).sum() > 0.5 * ticks * p.v_ref * p.dt   # it drove the course
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][2][0], runs[1][2][0])
    assert runs[0][2][1] == runs[1][2][1] and runs[0][2][5] == runs[1][2][5] == ticks


def test_resident_zero_dt_matches_host_prologue():
    """dt = 0 is defined in the reference (stride 0: the window is H copies of the nearest pose, dd:160-163) and admitted by
    the host prologue and the resident step alike: same index, same window, same u*, and the plant does not move."""
    p = configs.diff_drive_defaults(512, 20)
    px, py = amd.make_path("sinusoid")
    s0 = np.array([0.7, 0.1, 0.05])
    g = MPPIController(p)
    g.resident_set_path(px, py)
    g.resident_set_pose(s0)
    g.resident_step_enqueue(p.dt, 3, 0, advance=False)
    g.resident_step_enqueue(0.0, 3, 1, advance=True)
    u_res = g.get_nominal()
    st, idx, xr, yr, _, steps = g.resident_read()
    np.testing.assert_array_equal(st, s0)                      # dt = 0: the pose stays
    h = MPPIController(p)
    i0, wx, wy, wyaw = amd.calc_ref_path(px, py, s0[0], s0[1], p.v_ref, p.dt, p.resolution, p.horizon)
    h.iterate(s0, p.dt, wx, wy, wyaw[0], 3, 0, want_stats=False)
    i1, wx, wy, wyaw = amd.calc_ref_path(px, py, s0[0], s0[1], p.v_ref, 0.0, p.resolution, p.horizon)
    u_host = h.iterate(s0, 0.0, wx, wy, wyaw[0], 3, 1, want_stats=False)
    assert idx == i1 and steps == 2
    np.testing.assert_array_equal(xr, wx)
    np.testing.assert_array_equal(yr, wy)
    assert np.all(xr == xr[0])
    np.testing.assert_array_equal(u_res, u_host)

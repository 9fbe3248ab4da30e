"""GPU tests (-m gpu) of the batch handles' per-instance disc obstacles (ccv_mppi_batch_set_obstacles,
BatchController.set_obstacles).

The checker is tests/obstacle_reference.py: the penalty of the states the device itself stored (read_candidates) from the
real-arithmetic definition, with the bound of the device spec; cost_on - cost_off of the same handle, the same seeds and the
same warm start is held against it with bound_difference added (two differently rounded running sums).  Conditions on the
inputs are asserted: the discs are chosen on the CPU from the oracle's Philox rollouts -- one disc centred on a window point
near the middle of the horizon, its radius the median over the samples of the closest approach (discs_for) -- so that in every
instance with discs between 10 % and 90 % of the samples carry a non-zero reference penalty (found on the oracle's rollouts:
50 % - 56 % over the cases below; the device's shares are printed with -s).
"""
import numpy as np
import pytest

import batch_support as BS
import ccv_mppi_path_tracker_amd as amd
import helpers
import update_checks as UC
import update_reference as R
from batch_support import OV, SHIFT, same_bits, snapshot
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from obstacle_cases import CASES, NS, W_OBS, check_penalty, discs_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def run_off_on(p, B, inputs, discs, weights, shift, it=0):
    """one handle: term off, then on, from the same warm start and seeds -> (off, on, kernel off, kernel on, handle)"""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat = BatchController(p, B, min_shift=shift)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
    off, k_off = snapshot(bat, u, st), bat.last_kernel()
    bat.set_obstacles(discs, weights)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
    return off, snapshot(bat, u, st), k_off, bat.last_kernel(), bat


# 1. the term touches only the cost; nothing leaks; families --------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,K,H,B,over,fam", CASES)
def test_term_touches_only_the_cost(model, K, H, B, over, fam, shift):
    p = BS.MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**over)
    if fam == "solo":
        assert BS.families(model, K, B)[1] == "solo"
    inputs = BS.instance_inputs(p, B)
    ns = NS if B >= len(NS) else (3, 32)
    discs = discs_for(p, inputs, ns=ns)
    weights = np.full(B, W_OBS)
    if B >= len(NS):
        weights[3] = 0.0   # discs, but no weight
    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, discs, weights, shift)
    family = capi.BATCH_KERNEL_ONE_WAVE if fam == "solo" else capi.BATCH_KERNEL_FOUR_WAVE
    wide = capi.BATCH_KERNEL_WIDE if fam == "r4w" else 0
    assert k_off == family | wide | ((SHIFT | capi.BATCH_KERNEL_VARIED) if shift else 0)
    assert k_on == family | wide | OV | (SHIFT if shift else 0)
    for b in range(B):
        what = "%s K=%d H=%d %s b=%d n=%d%s" % (model, K, H, fam, b, len(discs[b]), " shift" if shift else "")
        check_penalty(what, p, inputs[0][b], discs[b], weights[b], off[b], on[b])
        if len(discs[b]) == 0 or weights[b] == 0.0:   # nothing leaks: fma(w, 0, cost) = cost exactly
            assert same_bits(off[b], on[b]), what
        else:
            assert not np.array_equal(off[b]["c"], on[b]["c"])
    # _set_obstacles(NULL) restores the kernel and every bit
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat.set_obstacles(None)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    back = snapshot(bat, u, st)
    assert bat.last_kernel() == k_off
    assert all(same_bits(off[b], back[b]) for b in range(B))
    bat.close()


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_plain_family_through_one_heading(shift):
    """one instance's heading outside the fast sin / cos range sends the batch through the plain kernel's OBST form"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    inputs[0][1, 2] += 2.0e5 * np.pi
    discs = discs_for(p, inputs)
    weights = np.full(B, W_OBS)
    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, discs, weights, shift)
    assert k_on == capi.BATCH_KERNEL_PLAIN | OV | (SHIFT if shift else 0)
    for b in range(B):
        check_penalty("plain b=%d n=%d" % (b, len(discs[b])), p, inputs[0][b], discs[b], weights[b], off[b], on[b])
        if len(discs[b]) == 0:
            assert same_bits(off[b], on[b])
    bat.close()


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_four_wave_and_one_wave_agree(shift, monkeypatch):
    """the same instances in a batch small enough for the four-wave kernel and in one large enough for the one-wave kernel
    (copies of the instances fill it up)"""
    K, H = 1000, 15
    p = configs.diff_drive_defaults(K, H)
    B4 = 5
    reps = -(-(5 * BS.cus() + 1) // (16 * B4))
    B1 = B4 * reps
    assert BS.families(p.model, K, B4)[1] == "r4" and BS.families(p.model, K, B1)[1] == "solo"
    inp = BS.instance_inputs(p, B4)
    discs = discs_for(p, inp)
    res = []
    for B, r in ((B4, 1), (B1, reps)):
        x0, dt, xr, yr, yaw0, seeds, nom = [np.concatenate([a] * r) for a in inp]
        bat = BatchController(p, B, min_shift=shift)
        bat.set_obstacles(discs * r, W_OBS)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res.append((u[:B4].copy(), [bat.read_costs(b) for b in range(B4)], bat.last_kernel()))
        bat.close()
    (u4, c4, k4), (u1, c1, k1) = res
    assert k4 == capi.BATCH_KERNEL_FOUR_WAVE | OV | (SHIFT if shift else 0)
    assert k1 == capi.BATCH_KERNEL_ONE_WAVE | OV | (SHIFT if shift else 0)
    for b in range(B4):
        assert helpers.rel_err(u4[b], u1[b]) < BS.TOL_U
        assert np.max(np.abs(c4[b] - c1[b]) / c1[b]) < BS.TOL_COST


def test_one_instances_discs_change_no_bit_of_another():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 5, 2
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs = discs_for(p, inputs)
    other = [d.copy() for d in discs]
    other[j] = other[j] + (0.2, -0.1, 0.3)
    snaps = []
    for d in (discs, other):
        bat = BatchController(p, B, min_shift=True)
        bat.set_obstacles(d, W_OBS)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        snaps.append(snapshot(bat, u, st))
        bat.close()
    assert not np.array_equal(snaps[0][j]["c"], snaps[1][j]["c"])
    for b in range(B):
        if b != j:
            assert same_bits(snaps[0][b], snaps[1][b])


# 2. the update -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_update_from_the_term_on_costs(shift):
    """u*, sum_w and n_zero_weight from the term-on costs inside update_reference's bounds: E_MAX with shift off (check_update
    measures E and caps it), E_SHIFT = 9 with shift on (update_checks.check_shift)"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs = discs_for(p, inputs)
    probe = BatchController(p, B)
    probe.set_obstacles(discs, W_OBS)
    probe.set_nominal(nom)
    probe.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    plist = [p.with_(lam=R.regime_lambda(probe.read_costs(b), "flat")) for b in range(B)]
    probe.close()
    bat = BatchController(plist, B, min_shift=shift)
    bat.set_obstacles(discs, W_OBS)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | OV | (SHIFT if shift else 0)
    for b in range(B):
        ctl = UC.host_controls(plist[b], nom[b], seeds[b], 0)
        what = "obstacles b=%d n=%d" % (b, len(discs[b]))
        if shift:
            UC.check_shift(what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b], sens=False)
        else:
            UC.check_update("batch obstacles", what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b],
                            sens=False)
    bat.close()


def test_hard_penalty_needs_the_shift():
    """instance 1: a disc of 50 m around its pose, weight 1e6 -- every sample penetrates by > 2000 m^2, every plain weight
    underflows: sum_w = 0, u* = NaN, flagged, its neighbours untouched; with shift on the same instance yields a finite u*"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 3
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs = [np.zeros((0, 3)), np.array([[x0[1, 0], x0[1, 1], 50.0]]), np.zeros((0, 3))]
    off, on, _, _, bat = run_off_on(p, B, inputs, discs, [0.0, 1e6, 0.0], False)
    assert np.all(on[1]["c"] > 1e6 * 2000.0)
    assert np.all(np.isnan(on[1]["u"])) and on[1]["st"][0] == 0.0 and on[1]["st"][4] == 1   # (sum_w, ..., nonfinite)
    assert same_bits(off[0], on[0]) and same_bits(off[2], on[2])
    bat.set_min_shift(True)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert np.all(np.isfinite(u)) and st[1].sum_w >= 1.0 and st[1].nonfinite == 0
    bat.close()


# 3. the resident loop ------------------------------------------------------------------------------------------------------
def test_resident_loop_with_discs_equals_the_host_prologue():
    """40 advancing ticks, B = 4, different discs per instance: pose, index, u* and costs of the resident batch equal the host
    prologue (calc_ref_path, plant_step) driving ccv_mppi_batch_iterate with the same discs, bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 4, 41
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    discs = []
    for b in range(B):
        i = (37 * b + 5) % (len(paths[b][0]) // 2) + 12 + 2 * b   # a path point ahead, inside the rollouts' reach from tick 0 on
        assert i + 10 < len(paths[b][0])   # (the sinusoid path has 101 points)
        discs.append(np.array([[paths[b][0][i], paths[b][1][i], 0.3 + 0.1 * b]] + [[paths[b][0][i + 10], paths[b][1][i + 10] + 1.0, 0.5]] * b))
    host = BatchController(p, B, min_shift=True)
    host.set_obstacles(discs, 50.0)
    s, u, ref = s0.copy(), None, []
    for it in range(ticks):
        if it > 0:
            s = np.array([amd.plant_step(p.model, s[b], u[b][0], p.dt) for b in range(B)])
        idx, xr, yr, yaw0 = np.zeros(B, dtype=np.int64), np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B)
        for b in range(B):
            idx[b], xr[b], yr[b], yaw = amd.calc_ref_path(paths[b][0], paths[b][1], s[b, 0], s[b, 1], p.v_ref, p.dt, p.resolution, p.horizon)
            yaw0[b] = yaw[0]
        u = host.iterate(s, p.dt, xr, yr, yaw0, seeds, it, want_stats=False)
        ref.append((s.copy(), idx, u.copy(), [host.read_costs(b) for b in range(B)] if it in (0, 20, ticks - 1) else None))
    host.close()
    bat = BatchController(p, B, min_shift=True)
    bat.set_obstacles(discs, 50.0)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        if it in (0, 20, ticks - 1):
            st, idx, _, _, _, steps = bat.resident_read()
            ws, widx, wu, wc = ref[it]
            assert steps == it + 1
            np.testing.assert_array_equal(st, ws)
            np.testing.assert_array_equal(idx, widx)
            np.testing.assert_array_equal(bat.get_nominal(), wu)
            for b in range(B):
                np.testing.assert_array_equal(bat.read_costs(b), wc[b])
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT
    bat.close()


def test_resident_robot_keeps_away_from_a_disc_on_its_path():
    """one disc centred on a path point ahead, shift on: the trace's smallest distance to the centre is strictly larger with
    the term on than with it off (two runs compared; the size of the gap is the tool's to record)"""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 2, 60
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    discs = []
    for b in range(B):
        i = (37 * b + 5) % (len(paths[b][0]) // 2) + 15   # (the robots cover 2.4 m and 4.4 m of path in 60 ticks)
        discs.append(np.array([[paths[b][0][i], paths[b][1][i], 0.4]]))
    closest = []
    for on in (False, True):
        bat = BatchController(p, B, min_shift=True)
        if on:
            bat.set_obstacles(discs, 200.0)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        closest.append([float(np.min(np.hypot(*(bat.resident_read_trace(b)[:, :2] - discs[b][0, :2]).T))) for b in range(B)])
        bat.close()
    print("closest approach off / on:", closest)
    for b in range(B):
        assert closest[0][b] < 0.4   # (the condition: with the term off the robot drives through the disc)
        assert closest[1][b] > closest[0][b]


# 4. refusals, flush, memory ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_get_round_trips():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs = discs_for(p, inputs)
    weights = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    bat = BatchController(p, B)
    got, w = bat.get_obstacles()
    assert all(g.shape == (0, 3) for g in got) and not w.any()
    bat.set_obstacles(discs, weights)
    got, w = bat.get_obstacles()
    for a, b in zip(got, discs):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(w, weights)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    want = snapshot(bat, u, st, states=False)
    lib, ip = bat.lib, lambda a: a.ctypes.data_as(capi.C.POINTER(capi.C.c_int32))

    def refused(xyr, n, max_n, wt):
        xyr, n, wt = np.ascontiguousarray(xyr, dtype=np.float64), np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(wt, dtype=np.float64)
        assert lib.ccv_mppi_batch_set_obstacles(bat._h, capi.dptr(xyr), ip(n), max_n, capi.dptr(wt)) == capi.ERR_INVALID_ARG

    ok = np.ones((B, 2, 3))
    one = np.ones(B, dtype=np.int32)
    for bad_w in (-1.0, np.nan, np.inf):
        refused(ok, one, 2, [1.0, bad_w, 1.0, 1.0, 1.0])
    for col, val in ((2, -0.5), (2, np.nan), (2, np.inf), (0, np.nan), (1, np.inf)):
        x = ok.copy()
        x[3, 0, col] = val
        refused(x, one, 2, np.ones(B))
    refused(ok, [1, 3, 1, 1, 1], 2, np.ones(B))
    refused(ok, [1, -1, 1, 1, 1], 2, np.ones(B))
    refused(np.ones((B, 33, 3)), one, 33, np.ones(B))
    got, w = bat.get_obstacles()
    for a, b in zip(got, discs):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(w, weights)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert all(same_bits(a, b, states=False) for a, b in zip(want, snapshot(bat, u, st, states=False)))
    # _set_params and _set_params(NULL) keep the obstacles
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert all(same_bits(a, b, states=False) for a, b in zip(want, snapshot(bat, u, st, states=False)))
    bat.close()


def test_set_obstacles_flushes_a_pending_resident_update():
    p = configs.diff_drive_defaults(1000, 15)
    B = 4
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    discs = [np.array([[paths[b][0][60], paths[b][1][60], 0.4]]) for b in range(B)]

    def run(sync):
        bat = BatchController(p, B, min_shift=True)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        out = []
        for it in range(6):
            if it == 3:
                bat.set_obstacles(discs, 100.0)   # (tick 2's update is pending here)
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if sync:
                bat.synchronize()
        out.append(bat.get_nominal())
        out.append(bat.resident_read()[0])
        k = bat.last_kernel()
        bat.close()
        return out, k

    (a, ka), (b, kb) = run(False), run(True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert ka == kb == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT


def test_obstacles_return_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)
    discs = [np.array([[1.0, 2.0, 0.5]] * (b % 4)).reshape(-1, 3) for b in range(B)]

    def cycle():
        bat = BatchController(p, B)
        bat.set_obstacles(discs, 1.0)
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
    bat = BatchController(p, B)
    bat.iterate(*inputs[:6], 0)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(200):
        bat.set_obstacles(discs if i % 2 == 0 else None, 1.0)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 2 * 2**20
    bat.close()

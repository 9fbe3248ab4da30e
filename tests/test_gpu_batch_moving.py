"""GPU tests (-m gpu) of the batch handles' moving discs (ccv_mppi_batch_set_obstacle_velocities,
BatchController.set_obstacles(..., velocities=), .set_obstacle_velocities).

The checker is tests/moving_obstacle_reference.py: the penalty of the states the device itself stored (read_candidates, row k =
state k, row 0 the pose) against discs at o + v k dt, from the real-arithmetic definition, with the bound of the device spec;
cost_moving - cost_off of the same handle, seeds and warm start is held against it with bound_difference added.  Conditions on
the inputs are asserted: disc 0 of every instance with discs is chosen on the CPU from the oracle's Philox rollouts so that
it is ON a window point near the middle of the horizon AT that point's step while moving at v_ref across the path, its radius
the median over the samples of the closest approach (moving_discs_for) -- between 10 % and 90 % of the samples carry a
reference penalty, and for at least 10 % of those the moving and the static reference penalty differ by more than ten times
the bound, so a kernel that ignores tau, or is a step late, cannot pass (on the oracle's rollouts: 50 % - 61 % and 100 % over
the cases below; the device's shares are printed with -s)."""
import numpy as np
import pytest

import batch_support as BS
import ccv_mppi_path_tracker_amd as amd
import fleet_reference as FR
import fleet_support as FS
import fleet_velocity_reference as FV
import helpers
import obstacle_cases as OC
import update_checks as UC
import update_reference as R
from batch_support import MOV, OV, SHIFT, same_bits, snapshot
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from fleet_support import CROSSING
from obstacle_cases import NS, W_OBS, check_moving, moving_discs_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def run_all(p, B, inputs, discs, vels, weights, shift, it=0):
    """one handle, the same warm start and seeds: term off, static discs, moving discs, a velocity table of zeros, velocities
    removed, discs removed -> the six snapshots, the six kernel codes"""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat = BatchController(p, B, min_shift=shift)
    snaps, codes = [], []

    def go():
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        snaps.append(snapshot(bat, u, st))
        codes.append(bat.last_kernel())

    go()
    bat.set_obstacles(discs, weights)
    go()
    bat.set_obstacle_velocities(vels)
    go()
    bat.set_obstacle_velocities([np.zeros_like(v) for v in vels])
    go()
    bat.set_obstacle_velocities(None)
    go()
    bat.set_obstacles(discs, weights, velocities=vels)   # (the one call; then the discs go, and the velocities with them)
    bat.set_obstacles(None)
    go()
    bat.close()
    return snaps, codes


def check_case(p, B, inputs, discs, vels, weights, shift, family, what0):
    snaps, codes = run_all(p, B, inputs, discs, vels, weights, shift)
    off, sta, mov, zero, unmoved, back = snaps
    base = family | ((SHIFT | capi.BATCH_KERNEL_VARIED) if shift else 0)
    sh = SHIFT if shift else 0
    assert codes == [base, family | OV | sh, family | MOV | sh, family | MOV | sh, family | OV | sh, base], (what0, codes)
    for b in range(B):
        what = "%s b=%d n=%d%s" % (what0, b, len(discs[b]), " shift" if shift else "")
        check_moving(what, p, inputs[0][b], inputs[1][b], discs[b], vels[b], weights[b], off[b], sta[b], mov[b])
        if len(discs[b]) == 0 or weights[b] == 0.0:   # an instance without discs, or without weight, keeps every bit
            assert same_bits(off[b], mov[b]), what
        else:
            assert not np.array_equal(sta[b]["c"], mov[b]["c"]), what
        # a table of zeros ran the MOVING kernels (codes) and gives the static term's bits; NULL restores kernel and bits
        assert same_bits(sta[b], zero[b]), what
        assert same_bits(sta[b], unmoved[b]), what
        assert same_bits(off[b], back[b]), what


# 1. - 3. the term touches only the cost; zero velocities; restoration ------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,K,H,B,over,fam", OC.CASES)
def test_moving_term_touches_only_the_cost(model, K, H, B, over, fam, shift):
    p = BS.MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**over)
    if fam == "solo":
        assert BS.families(model, K, B)[1] == "solo"
    inputs = BS.instance_inputs(p, B)
    ns = NS if B >= len(NS) else (3, 32)
    discs, vels = moving_discs_for(p, inputs, ns=ns)
    weights = np.full(B, W_OBS)
    if B >= len(NS):
        weights[3] = 0.0   # discs, but no weight
    family = (capi.BATCH_KERNEL_ONE_WAVE if fam == "solo" else capi.BATCH_KERNEL_FOUR_WAVE) | (capi.BATCH_KERNEL_WIDE if fam == "r4w" else 0)
    check_case(p, B, inputs, discs, vels, weights, shift, family, "%s K=%d H=%d %s" % (model, K, H, fam))


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_plain_family_through_one_heading(shift):
    """one instance's heading outside the fast sin / cos range sends the batch through the plain kernel's MOVING form"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    inputs[0][1, 2] += 2.0e5 * np.pi
    discs, vels = moving_discs_for(p, inputs)
    check_case(p, B, inputs, discs, vels, np.full(B, W_OBS), shift, capi.BATCH_KERNEL_PLAIN, "plain")


def test_one_instances_velocities_change_no_bit_of_another():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 5, 2
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs, vels = moving_discs_for(p, inputs)
    other = [v.copy() for v in vels]
    other[j] = other[j] * 0.5 + (0.1, -0.05)
    snaps = []
    for v in (vels, other):
        bat = BatchController(p, B, min_shift=True)
        bat.set_obstacles(discs, W_OBS, velocities=v)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        snaps.append(snapshot(bat, u, st))
        bat.close()
    assert not np.array_equal(snaps[0][j]["c"], snaps[1][j]["c"])
    for b in range(B):
        if b != j:
            assert same_bits(snaps[0][b], snaps[1][b])


# 4. four-wave against one-wave; the update ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_four_wave_and_one_wave_agree(shift):
    K, H = 1000, 15
    p = configs.diff_drive_defaults(K, H)
    B4 = 5
    reps = -(-(5 * BS.cus() + 1) // (16 * B4))
    B1 = B4 * reps
    assert BS.families(p.model, K, B4)[1] == "r4" and BS.families(p.model, K, B1)[1] == "solo"
    inp = BS.instance_inputs(p, B4)
    discs, vels = moving_discs_for(p, inp)
    res = []
    for B, r in ((B4, 1), (B1, reps)):
        x0, dt, xr, yr, yaw0, seeds, nom = [np.concatenate([a] * r) for a in inp]
        bat = BatchController(p, B, min_shift=shift)
        bat.set_obstacles(discs * r, W_OBS, velocities=vels * r)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res.append((u[:B4].copy(), [bat.read_costs(b) for b in range(B4)], bat.last_kernel()))
        bat.close()
    (u4, c4, k4), (u1, c1, k1) = res
    assert k4 == capi.BATCH_KERNEL_FOUR_WAVE | MOV | (SHIFT if shift else 0)
    assert k1 == capi.BATCH_KERNEL_ONE_WAVE | MOV | (SHIFT if shift else 0)
    for b in range(B4):
        assert helpers.rel_err(u4[b], u1[b]) < BS.TOL_U
        assert np.max(np.abs(c4[b] - c1[b]) / c1[b]) < BS.TOL_COST


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_update_from_the_moving_costs(shift):
    """u*, sum_w and n_zero_weight from the moving-term costs inside update_reference's bounds (E_MAX with shift off, E_SHIFT = 9
    with shift on, as test_gpu_batch_obstacles)"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs, vels = moving_discs_for(p, inputs)
    probe = BatchController(p, B)
    probe.set_obstacles(discs, W_OBS, velocities=vels)
    probe.set_nominal(nom)
    probe.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    plist = [p.with_(lam=R.regime_lambda(probe.read_costs(b), "flat")) for b in range(B)]
    probe.close()
    bat = BatchController(plist, B, min_shift=shift)
    bat.set_obstacles(discs, W_OBS, velocities=vels)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | MOV | (SHIFT if shift else 0)
    for b in range(B):
        ctl = UC.host_controls(plist[b], nom[b], seeds[b], 0)
        what = "moving b=%d n=%d" % (b, len(discs[b]))
        if shift:
            UC.check_shift(what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b], sens=False)
        else:
            UC.check_update("batch moving", what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b],
                            sens=False)
    bat.close()


# 5. the resident loop ------------------------------------------------------------------------------------------------------
def test_resident_loop_with_moving_discs_equals_the_host_prologue():
    """40 advancing ticks, B = 4, diff drive, different moving discs per instance: pose, index, u* and costs of the resident
    batch equal the host prologue driving ccv_mppi_batch_iterate with the same discs and velocities, bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 4, 41
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    discs, vels = [], []
    for b in range(B):
        i = (37 * b + 5) % (len(paths[b][0]) // 2) + 12 + 2 * b
        assert i + 10 < len(paths[b][0])
        discs.append(np.array([[paths[b][0][i], paths[b][1][i] - 0.5, 0.3 + 0.1 * b]] + [[paths[b][0][i + 10], paths[b][1][i + 10] + 1.0, 0.5]] * b))
        vels.append(np.array([[0.0, 0.7]] + [[-0.4, -0.6]] * b))
    host = BatchController(p, B, min_shift=True)
    host.set_obstacles(discs, 50.0, velocities=vels)
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
    bat.set_obstacles(discs, 50.0, velocities=vels)
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
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | MOV | SHIFT
    bat.close()


# 8. refusals, flush, memory ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_get_round_trips():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    discs, vels = moving_discs_for(p, inputs)
    bat = BatchController(p, B)
    lib = bat.lib
    some = np.ones((B, 2, 2))
    # no discs: CCV_MPPI_ERR_STATE, also for NULL; the getter gives zeros
    assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, capi.dptr(some), 2) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, None, 0) == capi.ERR_STATE
    assert all(v.shape == (0, 2) for v in bat.get_obstacle_velocities())
    bat.set_obstacles(discs, W_OBS)
    assert all(not v.any() and v.shape == (len(d), 2) for v, d in zip(bat.get_obstacle_velocities(), discs))
    bat.set_obstacle_velocities(vels)
    for a, b in zip(bat.get_obstacle_velocities(), vels):
        np.testing.assert_array_equal(a, b)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    want = snapshot(bat, u, st, states=False)
    big = np.ones((B, 32, 2))
    for bad in (np.nan, np.inf, -np.inf):
        x = big.copy()
        x[4, 31, 1] = bad          # (instance 4 has 32 discs: its last row counts)
        assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, capi.dptr(x), 32) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, capi.dptr(np.ones((B, 33, 2))), 33) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, capi.dptr(big), -1) == capi.ERR_INVALID_ARG
    out = np.zeros((B, 33, 2))
    assert lib.ccv_mppi_batch_get_obstacle_velocities(bat._h, capi.dptr(out), 33) == capi.ERR_INVALID_ARG
    # ... and none of the refused calls wrote anything or changed the kernel: the host copy, and every bit of a run
    for a, b in zip(bat.get_obstacle_velocities(), vels):
        np.testing.assert_array_equal(a, b)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() & capi.BATCH_KERNEL_MOVING
    assert all(same_bits(a, b, states=False) for a, b in zip(want, snapshot(bat, u, st, states=False)))
    x = big.copy()
    x[1, 5, 0] = np.nan            # a row past instance 1's count (one disc) is ignored
    assert lib.ccv_mppi_batch_set_obstacle_velocities(bat._h, capi.dptr(x), 32) == capi.OK
    assert bat.get_obstacle_velocities()[1].tolist() == [[1.0, 1.0]]
    bat.set_obstacle_velocities(vels)
    for a, b in zip(bat.get_obstacle_velocities(), vels):
        np.testing.assert_array_equal(a, b)
    # _set_params and _set_params(NULL) keep discs and velocities
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() & capi.BATCH_KERNEL_MOVING
    assert all(same_bits(a, b, states=False) for a, b in zip(want, snapshot(bat, u, st, states=False)))
    # a new list has no velocities until it is given some
    bat.set_obstacles(discs, W_OBS)
    assert all(not v.any() for v in bat.get_obstacle_velocities())
    bat.set_nominal(nom)
    bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() & (capi.BATCH_KERNEL_MOVING | capi.BATCH_KERNEL_OBST) == capi.BATCH_KERNEL_OBST
    bat.close()


def test_set_obstacle_velocities_flushes_a_pending_resident_update():
    p = configs.diff_drive_defaults(1000, 15)
    B = 4
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    discs = [np.array([[paths[b][0][60], paths[b][1][60] - 0.4, 0.4]]) for b in range(B)]
    vels = [np.array([[0.0, 0.5]]) for b in range(B)]

    def run(sync):
        bat = BatchController(p, B, min_shift=True)
        bat.set_obstacles(discs, 100.0)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        for it in range(6):
            if it == 3:
                bat.set_obstacle_velocities(vels)   # (tick 2's update is pending here)
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if sync:
                bat.synchronize()
        out = [bat.get_nominal(), bat.resident_read()[0]]
        k = bat.last_kernel()
        bat.close()
        return out, k

    (a, ka), (b, kb) = run(False), run(True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert ka == kb == capi.BATCH_KERNEL_FOUR_WAVE | MOV | SHIFT


def test_velocities_return_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)
    discs = [np.array([[1.0, 2.0, 0.5]] * (b % 4)).reshape(-1, 3) for b in range(B)]
    vels = [np.array([[0.3, -0.2]] * (b % 4)).reshape(-1, 2) for b in range(B)]

    def cycle():
        bat = BatchController(p, B)
        bat.set_obstacles(discs, 1.0, velocities=vels)
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
    bat.set_obstacles(discs, 1.0)
    bat.iterate(*inputs[:6], 0)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(200):
        bat.set_obstacle_velocities(vels if i % 2 == 0 else None)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 2 * 2**20
    bat.close()


# 6. fleet prediction against a twin handle ---------------------------------------------------------------------------------
def pred_twin_run(p, B, shift, static, static_v, radius, rng, maxn, weight, paths, s0, seeds, ticks, dts, advances):
    """the fleet term off: before every tick the lists from the poses read (fleet_reference), the velocities from the poses
    before and after the previous tick (fleet_velocity_reference), through set_obstacles and set_obstacle_velocities -> per
    tick (bits, n_total, disc table, velocity table)"""
    n_static = np.array([len(d) for d in static], dtype=np.int32)
    twin = FS.make(p, B, shift, None, weight, paths, s0, seeds)
    out, v = [], np.zeros((B, 2))
    for it in range(ticks):
        q = twin.resident_read()[0][:, :2]
        n_total, rows, taken = FV.lists(q, radius, n_static, maxn, rng)
        vrows = FV.velocity_rows(static_v, taken, v)
        twin.set_obstacles(FR.full_lists(static, rows), weight, velocities=vrows)
        twin.resident_step_enqueue(dts[it], it, advance=advances[it])
        out.append((FS.bits(twin), n_total, FR.table(static, rows), FV.table(vrows)))
        v = FV.velocity(q, twin.resident_read()[0][:, :2], dts[it], advances[it])
    k = twin.last_kernel()
    twin.close()
    return out, k


PRED_CASES = [("diff_drive", 15, False), ("diff_drive", 15, True), ("full_body", 10, False), ("full_body", 10, True)]


@pytest.mark.parametrize("model,H,shift", PRED_CASES, ids=["%s-H%d-%s" % (m[:2], h, "shift" if s else "plain_w") for m, h, s in PRED_CASES])
def test_fleet_prediction_equals_a_twin_fed_with_velocities(model, H, shift):
    """test_gpu_batch_fleet's fleet of five (max_neighbours = 2, static discs on two instances, 30 ticks) with prediction on: u*,
    costs, poses, indices, windows, the _read_fleet rows and the _read_fleet_velocities rows equal the twin's on every tick, read
    after every tick and, in a second run, at ticks 0, 14 and 29 only.  Tick 7 does not advance and, for diff drive, tick 11 has
    dt = 0: the velocities the ticks after them are charged with are zero (asserted on the tables)."""
    p = FS.params(model, 128, H)
    B, ticks, maxn, rng, weight = 5, 30, 2, 1.5, 50.0
    s0, seeds, paths = FS.fleet_start(p, B)
    static = [np.zeros((0, 3)), FS.far_discs(3), np.zeros((0, 3)), FS.far_discs(31, 1), np.zeros((0, 3))]
    static_v = [np.tile([0.3, -0.2], (len(d), 1)) for d in static]   # (static velocities beside the predicted ones)
    radius = np.array([0.15, 0.2, 0.1, 0.25, 0.3])
    dts = [p.dt] * ticks
    if model == "diff_drive":   # (full body refuses a resident step with dt = 0: it divides by dt)
        dts[11] = 0.0
    advances = [it > 0 and it != 7 for it in range(ticks)]
    want, k_twin = pred_twin_run(p, B, shift, static, static_v, radius, rng, maxn, weight, paths, s0, seeds, ticks, dts, advances)
    sv = FV.table(static_v)   # (the static rows: the caller's on every tick)
    assert (want[0][3] == sv).all() and (want[8][3] == sv).all()   # the first tick, and after a tick without advance: zero
    assert model != "diff_drive" or (want[12][3] == sv).all()      # after dt = 0: zero
    assert (want[5][3] != sv).any() and (want[20][3] != sv).any()  # ... and moving robots otherwise
    assert max(int((n - [0, 3, 0, 31, 0]).max()) for _, n, _, _ in want) == 2
    for every_tick in (True, False):
        bat = FS.make(p, B, shift, static, weight, paths, s0, seeds, fleet=(radius, rng, maxn, weight))
        bat.set_obstacle_velocities(static_v)
        assert not bat.resident_get_fleet_prediction()
        bat.resident_set_fleet_prediction(True)
        assert bat.resident_get_fleet_prediction()
        for it in range(ticks):
            bat.resident_step_enqueue(dts[it], it, advance=advances[it])
            if every_tick or it in (0, 14, ticks - 1):
                got = FS.bits(bat)
                ns, nt, xyr = bat.resident_read_fleet()
                vxy = bat.resident_read_fleet_velocities()
                wb, wn, wt, wv = want[it]
                for key in wb:
                    assert got[key] == wb[key], (key, it, every_tick)
                np.testing.assert_array_equal(nt, wn)
                assert xyr.tobytes() == wt.tobytes(), (it, every_tick)
                assert vxy.tobytes() == wv.tobytes(), (it, every_tick)
        assert bat.last_kernel() == k_twin == capi.BATCH_KERNEL_FOUR_WAVE | MOV | (SHIFT if shift else 0)
        bat.close()


def test_fleet_velocities_of_300_robots_equal_the_rule():
    """test_gpu_batch_fleet's grid of 300 robots (K = 64, H = 10, exact ties, n_static from {0, 30, 32}) with prediction: the
    velocity rows of every tick equal the rule on the poses read before and after the previous tick, beside the reference's
    selection"""
    p = FS.params("diff_drive", 64, 10)
    B, ticks, maxn, rng = 300, 8, 4, 0.6
    px, py = BS.path_of(0)
    s0 = np.zeros((B, p.nstate))
    s0[:, 0] = 1.0 + 0.25 * (np.arange(B) % 20)
    s0[:, 1] = 0.25 * (np.arange(B) // 20) - 1.75
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)
    n_static = np.array([0, 30, 0, 32, 0, 0, 30] * 43, dtype=np.int32)[:B]
    static = [FS.far_discs(int(n), b) for b, n in enumerate(n_static)]
    static_v = [np.zeros((int(n), 2)) for n in n_static]
    radius = 0.1 + 0.001 * np.arange(B)
    bat = FS.make(p, B, True, static, 20.0, (px, py), s0, seeds, fleet=(radius, rng, maxn, 20.0))
    bat.resident_set_fleet_prediction(True)
    q, v = s0[:, :2].copy(), np.zeros((B, 2))
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        n_total, rows, taken = FV.lists(q, radius, n_static, maxn, rng)
        ns, nt, xyr = bat.resident_read_fleet()
        np.testing.assert_array_equal(nt, n_total, err_msg="tick %d" % it)
        assert xyr.tobytes() == FR.table(static, rows).tobytes(), it
        want = FV.table(FV.velocity_rows(static_v, taken, v))
        assert bat.resident_read_fleet_velocities().tobytes() == want.tobytes(), it
        if it >= 2:
            assert want.any()
        q_after = bat.resident_read()[0][:, :2]
        v = FV.velocity(q, q_after, p.dt, it > 0)
        q = q_after
    bat.close()


def test_prediction_off_after_on_restores_every_bit_and_refusals():
    p = FS.params()
    B, ticks = 5, 8
    s0, seeds, paths = FS.fleet_start(p, B)
    fleet = (0.2, 1.5, 2, 50.0)

    def run(bat):
        bat.resident_set_poses(s0, seeds)
        bat.set_nominal(np.zeros((B, p.horizon - 1, p.udim)))
        out = []
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            out.append(FS.bits(bat))
        return out, bat.last_kernel()

    bat = FS.make(p, B, True, None, 50.0, paths, s0, seeds)
    # the fleet term off: the setter and the read are refused, nothing changes
    assert bat.lib.ccv_mppi_batch_set_fleet_prediction(bat._h, 1) == capi.ERR_STATE
    assert bat.lib.ccv_mppi_batch_read_fleet_velocities(bat._h, capi.dptr(np.zeros((B, 32, 2)))) == capi.ERR_STATE
    assert not bat.resident_get_fleet_prediction()
    bat.resident_set_fleet(*fleet)
    want, k0 = run(bat)
    assert k0 == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT and not bat.resident_read_fleet_velocities().any()
    bat.resident_set_fleet_prediction(True)
    on, k1 = run(bat)
    assert k1 == capi.BATCH_KERNEL_FOUR_WAVE | MOV | SHIFT and on != want and bat.resident_read_fleet_velocities().any()
    bat.resident_set_fleet_prediction(False)
    back, k2 = run(bat)
    assert k2 == k0 and back == want
    # turning the fleet term off turns prediction off
    bat.resident_set_fleet_prediction(True)
    bat.resident_set_fleet(None, 0.0, 0, None)
    assert not bat.resident_get_fleet_prediction()
    bat.resident_set_fleet(*fleet)
    assert not bat.resident_get_fleet_prediction()
    again, k3 = run(bat)
    assert k3 == k0 and again == want
    bat.close()


def test_prediction_off_with_static_velocities_leaves_no_neighbour_velocity():
    """Static discs with velocities that are not zero, the fleet term, then prediction on, off, on, and off by turning the fleet
    term off and on: every run without prediction equals, bit for bit and in the _read_fleet_velocities rows of every tick, a
    handle that never had prediction -- the MOVING kernels go on running there (the static velocities), and the rows of the
    neighbours' discs have to be zero again, not what the last tick with prediction left."""
    p = FS.params()
    B, ticks = 5, 8
    s0, seeds, paths = FS.fleet_start(p, B)
    fleet = (0.2, 1.5, 2, 50.0)
    px, py = paths[0]
    static = [np.zeros((0, 3)), FS.far_discs(3), np.array([[px[30], py[30] - 0.5, 0.3]]), FS.far_discs(5, 1), np.zeros((0, 3))]
    static_v = [np.zeros((0, 2)), np.tile([0.3, -0.2], (3, 1)), np.array([[0.0, 0.7]]), np.tile([-0.4, 0.6], (5, 1)), np.zeros((0, 2))]
    sv = FV.table(static_v)
    assert sv.shape == (B, 32, 2) and sv.any()

    def run(bat):
        bat.resident_set_poses(s0, seeds)
        bat.set_nominal(np.zeros((B, p.horizon - 1, p.udim)))
        out = []
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            out.append((FS.bits(bat), bat.resident_read_fleet()[1].tolist(), bat.resident_read_fleet_velocities().tobytes()))
        return out, bat.last_kernel()

    def make():
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=fleet)
        bat.set_obstacle_velocities(static_v)
        return bat

    never = make()
    want, k0 = run(never)
    never.close()
    assert k0 == capi.BATCH_KERNEL_FOUR_WAVE | MOV | SHIFT
    assert all(v == sv.tobytes() for _, _, v in want)              # the static rows the caller's, every other row zero
    assert max(max(n) for _, n, _ in want) > 5                     # ... beside neighbours' discs
    bat = make()
    first, k = run(bat)
    assert k == k0 and first == want
    bat.resident_set_fleet_prediction(True)
    on, k = run(bat)
    assert k == k0 and on != want and any(v != sv.tobytes() for _, _, v in on)
    bat.resident_set_fleet_prediction(False)
    back, k = run(bat)
    assert k == k0 and back == want
    bat.resident_set_fleet_prediction(True)
    on2, k = run(bat)
    assert on2 == on
    bat.resident_set_fleet(None, 0.0, 0, None)                     # (prediction goes off with the fleet term)
    bat.resident_set_fleet(*fleet)
    assert not bat.resident_get_fleet_prediction()
    again, k = run(bat)
    assert k == k0 and again == want
    bat.close()


# 7. behaviour: a crossing ----------------------------------------------------------------------------------------------------
def test_two_robots_crossing_pass_at_a_larger_distance_with_prediction():
    """Two robots on perpendicular straight paths, each 1.5 m from the crossing and timed to reach it together, K = 128, shifted
    weights, radii 0.1 m + 0.1 m, range 3 m, weight 100, 60 ticks: the closest approach (same tick) with predicted discs is
    larger than with snapshot discs by the CPU test's margin.  (The figures are printed with -s)"""
    p = FS.params()
    c = CROSSING
    B, ticks = 2, c["ticks"]
    closest = {}
    for mode in ("off", "snapshot", "predicted"):
        bat = FS.make(p, B, True, None, 0.0, c["paths"], c["s0"], c["seeds"],
                      fleet=(c["radius"], c["range"], 1, c["weight"]) if mode != "off" else None)
        if mode == "predicted":
            bat.resident_set_fleet_prediction(True)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        t0, t1 = bat.resident_read_trace(0), bat.resident_read_trace(1)
        assert len(t0) == len(t1) == ticks
        closest[mode] = float(np.min(np.hypot(*(t0[:, :2] - t1[:, :2]).T)))
        bat.close()
    print("closest approach off / snapshot / predicted: %.4f / %.4f / %.4f" % (closest["off"], closest["snapshot"], closest["predicted"]))
    assert closest["predicted"] > closest["snapshot"] + c["margin"]

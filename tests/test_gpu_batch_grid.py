"""GPU tests (-m gpu) of the batch handles' occupancy-grid term (ccv_mppi_batch_set_grids, BatchController.set_grids;
DESIGN.md section 10h).

The checker is tests/grid_reference.py: the term is made of IEEE basic operations on the states the device itself stored, so
cost_on is held against fma(w_grid, G_ref, cost_off) BIT FOR BIT, with G_ref the numpy restatement fed with the read-back states
(read_candidates) and cost_off the term-off run of the same handle, seeds and warm start.  Conditions on the inputs are asserted
on those states: every instance with a map has at least 25 % of its covered states in bounds, at least 5 % out of bounds and at
least 50 distinct cells hit (tests/test_grid_reference.py checks the same on the oracle's rollouts, without a GPU).

Instances of a batch of five, in order: no map; map 0; map 1; map 0 with weight 0; map 1 with another weight.  Instances 3 and 4
stand near instances 1 and 2 (grid_inputs), whose poses place the maps (grid_reference.map_ahead).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import batch_support as BS
import ccv_mppi_path_tracker_amd as amd
import fleet_support as FS
import grid_reference as GR
import helpers
import obstacle_cases as OC
import update_checks as UC
import update_reference as R
from batch_support import GRID, MOV, OV, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from grid_cases import CASES, PLAIN_CASE, check_identity, grid_inputs, maps_for, roles

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import grid_wall_cpu as GW  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def set_maps(bat, maps, map_of, w):
    bat.set_grids([g.as_tuple() for g in maps], map_of, w)


def run_off_on(p, B, inputs, maps, map_of, w, shift, prepare=None, it=0):
    """one handle: term off, then on, from the same warm start and seeds -> (off, on, kernel off, kernel on, handle)"""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat = BatchController(p, B, min_shift=shift)
    if prepare:
        prepare(bat)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
    off, k_off = BS.snapshot(bat, u, st), bat.last_kernel()
    set_maps(bat, maps, map_of, w)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
    return off, BS.snapshot(bat, u, st), k_off, bat.last_kernel(), bat


def check_all(what0, p, inputs, maps, map_of, w, off, on):
    for b in range(len(map_of)):
        what = "%s b=%d map=%d w=%g" % (what0, b, map_of[b], w[b])
        if map_of[b] < 0:
            assert BS.same_bits(off[b], on[b]), what
            continue
        check_identity(what, p, maps[map_of[b]], w[b], off[b], on[b])
        if w[b] == 0.0:
            assert BS.same_bits(off[b], on[b]), what
        else:
            assert not np.array_equal(off[b]["c"], on[b]["c"]), what


# 1. the spec, bit for bit; nothing else changes; families ------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,K,H,B,over,fam", CASES)
def test_grid_term_is_the_spec_bit_for_bit(model, K, H, B, over, fam, shift):
    p = BS.MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**over)
    if fam == "solo":
        assert BS.families(model, K, B)[1] == "solo"
    inputs = grid_inputs(p, B)
    maps, map_of, w = maps_for(p, inputs)
    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, maps, map_of, w, shift)
    family = capi.BATCH_KERNEL_ONE_WAVE if fam == "solo" else capi.BATCH_KERNEL_FOUR_WAVE
    wide = capi.BATCH_KERNEL_WIDE if fam == "r4w" else 0
    assert k_off == family | wide | ((SHIFT | capi.BATCH_KERNEL_VARIED) if shift else 0)
    assert k_on == family | wide | GRID | (SHIFT if shift else 0)
    check_all("%s K=%d H=%d %s%s" % (model, K, H, fam, " shift" if shift else ""), p, inputs, maps, map_of, w, off, on)
    # _set_grids(NULL) restores the kernel and every bit, twice over
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    for again in range(2):
        bat.set_grids(None)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        back = BS.snapshot(bat, u, st)
        assert bat.last_kernel() == k_off
        assert all(BS.same_bits(off[b], back[b]) for b in range(B))
        if again == 0:
            set_maps(bat, maps, map_of, w)
            bat.set_nominal(nom)
            u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
            assert bat.last_kernel() == k_on
            assert all(BS.same_bits(on[b], s) for b, s in enumerate(BS.snapshot(bat, u, st)))
    bat.close()


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_plain_family_through_one_heading(shift):
    """one instance's heading outside the fast sin / cos range sends the batch through the plain kernel's GRID form"""
    model, K, H, B, _, _ = PLAIN_CASE
    p = BS.MODEL_DEFAULTS[model](K, H)
    inputs = grid_inputs(p, B)
    inputs[0][0, 2] += 2.0e5 * np.pi   # (instance 0 has no map: no map is placed from this heading)
    maps, map_of, w = maps_for(p, inputs)
    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, maps, map_of, w, shift)
    assert k_on == capi.BATCH_KERNEL_PLAIN | GRID | (SHIFT if shift else 0)
    check_all("plain%s" % (" shift" if shift else ""), p, inputs, maps, map_of, w, off, on)
    bat.close()


def test_full_body_beyond_one_workgroup_per_cu_runs_the_four_wave_form():
    """The one-wave full-body kernel has no grid form (no register left): a full-body batch of that size
    runs the four-wave GRID form.  The term-off run is the one-wave kernel's, so the identity is held within TOL_COST instead
    of bit for bit: cost_on against fma(w, G_ref, cost_off) with G_ref from the term-on run's own states."""
    K, H = 128, 15
    p = configs.full_body_defaults(K, H)
    B = 5 * (BS.cus() // 10 + 1)   # (two workgroups per instance: more than one per CU)
    assert BS.families(p.model, K, B)[1] == "solo"
    inputs = grid_inputs(p, B)
    maps, map_of, w = maps_for(p, inputs)
    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, maps, map_of, w, False)
    assert k_off == capi.BATCH_KERNEL_ONE_WAVE and k_on == capi.BATCH_KERNEL_FOUR_WAVE | GRID
    for b in range(5):
        if map_of[b] < 0:
            continue
        P = on[b]["xy"][:, :GR.n_covered(p.model, H)]
        want = GR.cost_on(off[b]["c"], w[b], GR.grid_sum(maps[map_of[b]], P))
        assert np.max(np.abs(on[b]["c"] - want) / np.abs(want)) < BS.TOL_COST, b
    bat.close()


# 2. with discs, velocities, the fleet term and prediction ------------------------------------------------------------------
@pytest.mark.parametrize("vel", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_identity_holds_beside_discs(shift, vel):
    """discs (n = 0, 3, 32 dealt round), standing or moving: the grid-off run is the OBST / MOVING kernel with the same discs"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = grid_inputs(p, B)
    maps, map_of, w = maps_for(p, inputs)
    discs = OC.discs_for(p, inputs, ns=(32, 0, 3, 3, 32))
    vels = [np.stack([0.3 * np.cos(np.arange(len(d)) + b), 0.2 * np.sin(np.arange(len(d)) - b)], axis=1).reshape(-1, 2) for b, d in enumerate(discs)]

    def prepare(bat):
        bat.set_obstacles(discs, OC.W_OBS, velocities=vels if vel else None)

    off, on, k_off, k_on, bat = run_off_on(p, B, inputs, maps, map_of, w, shift, prepare)
    assert k_off == capi.BATCH_KERNEL_FOUR_WAVE | (MOV if vel else OV) | (SHIFT if shift else 0)
    assert k_on == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    check_all("discs%s%s" % (" moving" if vel else "", " shift" if shift else ""), p, inputs, maps, map_of, w, off, on)
    # the discs stay through _set_grids; the setters of the discs keep the maps
    got, _ = bat.get_obstacles()
    assert all(np.array_equal(a, b) for a, b in zip(got, discs))
    bat.set_obstacles(discs, OC.W_OBS, velocities=vels if vel else None)
    bat.set_min_shift(not shift)
    bat.set_min_shift(shift)
    bat.set_params([p] * B)
    bat.set_params(None)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() == k_on
    assert all(BS.same_bits(on[b], s) for b, s in enumerate(BS.snapshot(bat, u, st)))
    bat.close()


@pytest.mark.parametrize("pred", [False, True], ids=["snapshot", "predicted"])
def test_identity_holds_beside_the_fleet_term(pred):
    """two resident fleets run three ticks alike; then one gets the maps: its fourth tick's costs are the other's plus the term"""
    p = FS.params("diff_drive", 1000, 15)
    B = 5
    s0, seeds, paths = FS.fleet_start(p, B)
    map_of, w = roles(B)
    maps = [GR.map_ahead(s0[1, :3], p.v_ref, p.dt, p.horizon, salt=0), GR.map_ahead(s0[2, :3], p.v_ref, p.dt, p.horizon, salt=1)]
    static = [FS.far_discs(b % 3, b) for b in range(B)]
    res = []
    for on in (False, True):
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0)))
        if pred:
            bat.resident_set_fleet_prediction(True)
        for it in range(3):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        if on:
            set_maps(bat, maps, map_of, w)
        bat.resident_step_enqueue(p.dt, 3, advance=True)
        res.append(([dict(c=bat.read_costs(b), xy=bat.read_candidates(b)) for b in range(B)], bat.last_kernel(), bat.resident_read()[0]))
        bat.close()
    (off, k_off, s_off), (on, k_on, s_on) = res
    assert k_off == capi.BATCH_KERNEL_FOUR_WAVE | (MOV if pred else OV) | SHIFT and k_on == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    np.testing.assert_array_equal(s_off, s_on)
    for b in range(B):
        if map_of[b] < 0:
            assert off[b]["c"].tobytes() == on[b]["c"].tobytes() and off[b]["xy"].tobytes() == on[b]["xy"].tobytes()
        else:   # (the robots have moved on from the poses the maps were placed at: no coverage conditions here)
            check_identity("fleet%s b=%d" % (" pred" if pred else "", b), p, maps[map_of[b]], w[b], off[b], on[b], conditions=False)


def test_one_instances_map_changes_no_bit_of_another():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 5, 2
    inputs = grid_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    maps, map_of, w = maps_for(p, inputs)
    shifted = GR.Grid(maps[1].cells[::-1].copy(), (maps[1].ox + 0.07, maps[1].oy - 0.04), maps[1].resolution * 1.1, 9.0)
    variants = [(maps, map_of, w),
                (maps + [shifted], np.where(np.arange(B) == j, 2, map_of).astype(np.int32), w),      # another map
                (maps, np.where(np.arange(B) == j, 0, map_of).astype(np.int32), w),                   # another map_of
                (maps, map_of, np.where(np.arange(B) == j, 0.5, w))]                                  # another weight
    snaps = []
    for m, mo, wt in variants:
        bat = BatchController(p, B, min_shift=True)
        set_maps(bat, m, mo, wt)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        snaps.append(BS.snapshot(bat, u, st))
        bat.close()
    for s in snaps[1:]:
        assert not np.array_equal(snaps[0][j]["c"], s[j]["c"])
        for b in range(B):
            if b != j:
                assert BS.same_bits(snaps[0][b], s[b])


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_four_wave_and_one_wave_agree(shift):
    K, H = 1000, 15
    p = configs.diff_drive_defaults(K, H)
    B4 = 5
    reps = -(-(5 * BS.cus() + 1) // (16 * B4))
    B1 = B4 * reps
    assert BS.families(p.model, K, B4)[1] == "r4" and BS.families(p.model, K, B1)[1] == "solo"
    inp = grid_inputs(p, B4)
    maps, map_of, w = maps_for(p, inp)
    res = []
    for B, r in ((B4, 1), (B1, reps)):
        x0, dt, xr, yr, yaw0, seeds, nom = [np.concatenate([a] * r) for a in inp]
        bat = BatchController(p, B, min_shift=shift)
        set_maps(bat, maps, np.concatenate([map_of] * r), np.concatenate([w] * r))
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res.append((u[:B4].copy(), [bat.read_costs(b) for b in range(B4)], bat.last_kernel()))
        bat.close()
    (u4, c4, k4), (u1, c1, k1) = res
    assert k4 == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    assert k1 == capi.BATCH_KERNEL_ONE_WAVE | GRID | (SHIFT if shift else 0)
    for b in range(B4):
        assert helpers.rel_err(u4[b], u1[b]) < BS.TOL_U
        assert np.max(np.abs(c4[b] - c1[b]) / c1[b]) < BS.TOL_COST


# 3. the update -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
def test_update_from_the_term_on_costs(shift):
    """u*, sum_w and n_zero_weight from the term-on costs inside update_reference's bounds (as test_gpu_batch_obstacles.py)"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = grid_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    maps, map_of, w = maps_for(p, inputs)
    probe = BatchController(p, B)
    set_maps(probe, maps, map_of, w)
    probe.set_nominal(nom)
    probe.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    plist = [p.with_(lam=R.regime_lambda(probe.read_costs(b), "flat")) for b in range(B)]
    probe.close()
    bat = BatchController(plist, B, min_shift=shift)
    set_maps(bat, maps, map_of, w)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    for b in range(B):
        ctl = UC.host_controls(plist[b], nom[b], seeds[b], 0)
        what = "grid b=%d" % b
        if shift:
            UC.check_shift(what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b], sens=False)
        else:
            UC.check_update("batch grid", what, bat.read_costs(b), ctl, plist[b].lam, u[b], st[b].sum_w, bat.read_weights(b), st[b],
                            sens=False)
    bat.close()


def test_a_weight_that_underflows_needs_the_shift():
    """instance 1: every state reads at least 1, weight 1e6: every plain weight underflows -- sum_w = 0, u* = NaN, flagged, in
    that instance only; with shift on the same instance yields a finite u*"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 3
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    g = GR.Grid(1.0 + np.arange(35, dtype=np.float32).reshape(5, 7), (x0[1, 0] - 0.1, x0[1, 1] - 0.1), 0.05, 2.0)
    off, on, _, _, bat = run_off_on(p, B, inputs, [g], np.array([-1, 0, -1], dtype=np.int32), np.array([0.0, 1e6, 0.0]), False)
    assert np.all(on[1]["c"] > 1e6 * p.horizon)
    assert np.all(np.isnan(on[1]["u"])) and on[1]["st"][0] == 0.0 and on[1]["st"][4] == 1   # (sum_w, ..., nonfinite)
    assert BS.same_bits(off[0], on[0]) and BS.same_bits(off[2], on[2])
    bat.set_min_shift(True)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert np.all(np.isfinite(u)) and st[1].sum_w >= 1.0 and st[1].nonfinite == 0
    bat.close()


# 4. the resident loop ------------------------------------------------------------------------------------------------------
def resident_maps(p, B, s0):
    """two maps over the first metres of robots 1 and 2, large enough that 40 ticks stay in touch with them"""
    maps = [GR.map_ahead(s0[b, :3], p.v_ref, p.dt, p.horizon, salt=b - 1, ahead=2.0) for b in (1, 2)]
    return maps, np.array([-1, 0, 1, 0][:B], dtype=np.int32), np.array([0.0, 0.01, 0.02, 0.0][:B])


def test_resident_loop_with_maps_equals_the_host_prologue():
    """40 advancing ticks, B = 4, two maps: pose, index, u* and costs of the resident batch equal the host prologue
    (calc_ref_path, plant_step) driving ccv_mppi_batch_iterate with the same maps, bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 4, 41
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    maps, map_of, w = resident_maps(p, B, s0)
    host = BatchController(p, B, min_shift=True)
    set_maps(host, maps, map_of, w)
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
    assert host.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    host.close()
    bat = BatchController(p, B, min_shift=True)
    set_maps(bat, maps, map_of, w)
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
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    # the maps acted: the costs of a robot with a map differ from a run without
    plain = BatchController(p, B, min_shift=True)
    plain.resident_set_paths(paths)
    plain.resident_set_poses(s0, seeds)
    plain.resident_step_enqueue(p.dt, 0, advance=False)
    assert not np.array_equal(plain.read_costs(1), ref[0][3][1]) and np.array_equal(plain.read_costs(0), ref[0][3][0])
    plain.close()
    bat.close()


def test_a_wall_across_the_path_is_driven_round():
    """One robot on a straight path, shifted weights, K = 128; a block of occupied cells lies across the path and extends to one
    side only (tools/grid_wall_cpu.py: block, inflation ring and weight chosen on the CPU restatement of the closed loop,
    tests/test_grid_wall_cpu.py).  With the term off some trace poses lie in occupied cells; with it on none do.  (The size of
    the detour is printed with -s)"""
    p = configs.diff_drive_defaults(GW.SAMPLES, 15)
    g = GW.wall_map(**GW.WALL)
    s0, seeds = np.array([GW.START]), np.array([GW.SEED], dtype=np.uint64)
    inside = []
    for on in (False, True):
        bat = BatchController(p, 1, min_shift=True)
        if on:
            bat.set_grids([g.as_tuple()], [0], GW.WEIGHT)
        bat.resident_set_paths([GW.path()])
        bat.resident_set_poses(s0, seeds)
        for it in range(GW.TICKS):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        trace = bat.resident_read_trace(0)[:, :2]
        assert len(trace) == GW.TICKS
        assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | SHIFT | (GRID if on else capi.BATCH_KERNEL_VARIED)
        inside.append(GW.occupied(g, trace))
        print("term %s: %d poses in occupied cells, largest |y| %.3f m, end x %.2f" % ("on" if on else "off", inside[-1],
                                                                                      float(np.max(np.abs(trace[:, 1]))), trace[-1, 0]))
        bat.close()
    assert inside[0] > 0    # (the condition: with the term off the robot drives through the block)
    assert inside[1] == 0


# 5. refusals, round trips, flush, memory -----------------------------------------------------------------------------------
def test_refusals_change_nothing_and_get_round_trips():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = grid_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    maps, map_of, w = maps_for(p, inputs)
    bat = BatchController(p, B)
    got, mo, wt = bat.get_grids()
    assert got == [] and np.all(mo == -1) and not wt.any()
    lib, ip = bat.lib, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ccv_mppi_batch_read_grid_cells(bat._h, 0, maps[0].cells.ctypes.data_as(C.POINTER(C.c_float))) == capi.ERR_STATE
    set_maps(bat, maps, map_of, w)

    def holds():
        got, mo, wt = bat.get_grids()
        assert len(got) == 2 and np.array_equal(mo, map_of) and np.array_equal(wt, w)
        for (cells, origin, res, outside), g in zip(got, maps):
            assert cells.tobytes() == g.cells.tobytes() and cells.shape == (g.ny, g.nx)
            assert origin == (g.ox, g.oy) and res == g.resolution and outside == float(g.outside)

    holds()
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    want = BS.snapshot(bat, u, st, states=False)

    def refused(rows, n, mo, wt):
        mo, wt = np.ascontiguousarray(mo, dtype=np.int32), np.ascontiguousarray(wt, dtype=np.float64)
        assert lib.ccv_mppi_batch_set_grids(bat._h, rows, n, ip(mo), capi.dptr(wt)) == capi.ERR_INVALID_ARG

    def rows_of(**bad):
        cells = np.ones((3, 4), dtype=np.float32)
        cells.flat[bad.pop("cell_at", 0)] = bad.pop("cell", 1.0)
        keep.append(cells)
        f = dict(origin_x=0.0, origin_y=0.0, resolution=0.1, outside=-1.0, nx=4, ny=3, cells=cells.ctypes.data_as(C.POINTER(C.c_float)))
        f.update(bad)
        return (capi.Grid * 1)(capi.Grid(f["origin_x"], f["origin_y"], f["resolution"], f["outside"], f["nx"], f["ny"], f["cells"]))

    keep, ok_mo, ok_w = [], np.zeros(B, dtype=np.int32), np.ones(B)
    refused(rows_of(cells=C.POINTER(C.c_float)()), 1, ok_mo, ok_w)                       # null cells
    for nx, ny in ((0, 3), (4, 0), (-1, 3), (32769, 1), (1, 32769), (16384, 8192)):      # sizes out of range (the last: 2^27 cells)
        refused(rows_of(nx=nx, ny=ny), 1, ok_mo, ok_w)
    for res in (0.0, -0.1, np.nan, np.inf):
        refused(rows_of(resolution=res), 1, ok_mo, ok_w)
    for field in ("origin_x", "origin_y", "outside"):
        for v in (np.nan, np.inf, -np.inf):
            refused(rows_of(**{field: v}), 1, ok_mo, ok_w)
    for v in (np.nan, np.inf):
        refused(rows_of(cell=v, cell_at=11), 1, ok_mo, ok_w)                             # a non-finite cell, the last one
    for bad_w in (-1.0, np.nan, np.inf):
        refused(rows_of(), 1, ok_mo, [1.0, bad_w, 1.0, 1.0, 1.0])
    for bad_m in (-2, 1, 7):
        refused(rows_of(), 1, [0, 0, bad_m, 0, 0], ok_w)
    refused(rows_of(), -1, ok_mo, ok_w)
    assert lib.ccv_mppi_batch_set_grids(bat._h, rows_of(), 1, None, capi.dptr(ok_w)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_grid_cells(bat._h, 2, maps[0].cells.ctypes.data_as(C.POINTER(C.c_float))) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_grids(bat._h, rows_of(), 1, None, None, None) == capi.ERR_INVALID_ARG   # two maps, room for one
    holds()
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, BS.snapshot(bat, u, st, states=False)))
    # _set_params and _set_params(NULL) keep the maps
    bat.set_params([p] * B)
    bat.set_params(None)
    holds()
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
    assert all(BS.same_bits(a, b, states=False) for a, b in zip(want, BS.snapshot(bat, u, st, states=False)))
    bat.close()


def test_set_grids_flushes_a_pending_resident_update():
    p = configs.diff_drive_defaults(1000, 15)
    B = 4
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    maps, map_of, w = resident_maps(p, B, s0)

    def run(sync):
        bat = BatchController(p, B, min_shift=True)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        for it in range(6):
            if it == 3:
                set_maps(bat, maps, map_of, w)   # (tick 2's update is pending here)
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
    assert ka == kb == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT


def test_grids_return_all_device_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = grid_inputs(p, B)
    map_of, w = roles(B)
    big = GR.Grid(np.ones((700, 900), dtype=np.float32), (0.0, 0.0), 0.05, 0.0)   # (2.4 MiB: a leak per cycle would show)
    small = GR.Grid(np.ones((3, 5), dtype=np.float32), (0.0, 0.0), 0.05, 0.0)

    def cycle():
        bat = BatchController(p, B)
        set_maps(bat, [big, small], map_of, w)
        set_maps(bat, [small, big], map_of, w)   # (a new set is a new allocation: the old one must go)
        bat.iterate(*inputs[:6], 0)
        bat.close()

    for _ in range(3):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)

"""GPU tests (-m gpu) of the batch handles' fleet term (ccv_mppi_batch_resident_set_fleet, BatchController.resident_set_fleet;
DESIGN.md section 10f): the robots of one resident batch become discs of each other's obstacle lists, formed on the device in
the prologue of every tick.

The checker is tests/fleet_reference.py (pinned by tests/test_fleet_reference.py).  The term adds no cost arithmetic, so the
whole of it is held against existing code bit for bit: a twin handle with the term off reads the poses before every tick,
forms the lists with the reference, hands static + fleet discs to set_obstacles and steps.
"""
import numpy as np
import pytest

import batch_support as BS
import fleet_reference as FR
from batch_support import OV, SHIFT
from ccv_mppi_path_tracker_amd import capi
from ccv_mppi_path_tracker_amd.controller import MPPIError
from fleet_support import HEAD_ON, bits, far_discs, fleet_start, make, params, robot_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def twin_run(p, B, shift, static, radius, rng, maxn, weight, paths, s0, seeds, ticks, timed=False):
    """the term off; before every tick the lists from the poses read, through set_obstacles -> per tick (bits, n_total, table)"""
    n_static = np.array([len(d) for d in static], dtype=np.int32)
    twin = make(p, B, shift, None, weight, paths, s0, seeds, timed=timed)
    out = []
    for it in range(ticks):
        q = twin.resident_read()[0][:, :2]
        n_total, rows = FR.lists(q, radius, n_static, maxn, rng)
        twin.set_obstacles(FR.full_lists(static, rows), weight)
        twin.resident_step_enqueue(p.dt, it, advance=it > 0)
        out.append((bits(twin), n_total, FR.table(static, rows)))
    k = twin.last_kernel()
    twin.close()
    return out, k


# 1. the whole term against existing code, bit for bit ---------------------------------------------------------------------
WHOLE = [("diff_drive", 15, False, False), ("diff_drive", 15, True, False), ("steering_diff_drive", 10, False, False),
         ("steering_diff_drive", 10, True, False), ("full_body", 10, False, False), ("full_body", 10, True, False),
         ("diff_drive", 15, True, True)]


@pytest.mark.parametrize("model,H,shift,timed", WHOLE, ids=["%s-H%d-%s%s" % (m[:2], h, "shift" if s else "plain_w", "-timed" if t else "")
                                                            for m, h, s, t in WHOLE])
def test_fleet_equals_a_twin_fed_through_set_obstacles(model, H, shift, timed):
    """B = 5 on the sinusoid path within range of each other, max_neighbours = 2, static discs on two instances (n = 3, and
    n = 31 so that M_y = 1), 30 advancing ticks.  u*, costs, poses, indices, windows and the _read_fleet rows equal the twin's on
    every tick, read after every tick (the prologue kernel of its own) and, in a second run, only at ticks 0, 14 and 29 (the
    update launches that carry the prologue)."""
    p = params(model, 128, H)
    B, ticks, maxn, rng, weight = 5, 30, 2, 1.5, 50.0
    s0, seeds, paths = fleet_start(p, B)
    static = [np.zeros((0, 3)), far_discs(3), np.zeros((0, 3)), far_discs(31, 1), np.zeros((0, 3))]
    radius = np.array([0.15, 0.2, 0.1, 0.25, 0.3])
    want, k_twin = twin_run(p, B, shift, static, radius, rng, maxn, weight, paths, s0, seeds, ticks, timed)
    assert max(int((n - [0, 3, 0, 31, 0]).max()) for _, n, _ in want) == 2 and all(n[3] == 32 for _, n, _ in want)   # the inputs' condition
    for every_tick in ((True,) if timed else (True, False)):
        bat = make(p, B, shift, static, weight, paths, s0, seeds, fleet=(radius, rng, maxn, weight), timed=timed)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if every_tick or it in (0, 14, ticks - 1):
                got = bits(bat)
                ns, nt, xyr = bat.resident_read_fleet()
                wb, wn, wt = want[it]
                for key in wb:
                    assert got[key] == wb[key], (key, it, every_tick)
                np.testing.assert_array_equal(ns, [0, 3, 0, 31, 0])
                np.testing.assert_array_equal(nt, wn)
                assert xyr.tobytes() == wt.tobytes(), (it, every_tick)
        assert bat.last_kernel() == k_twin == capi.BATCH_KERNEL_FOUR_WAVE | OV | (SHIFT if shift else 0)
        bat.close()


# 2. no candidate, no change ---------------------------------------------------------------------------------------------------
def test_no_candidate_changes_no_bit():
    """range = 0 with the robots apart: every bit over 20 ticks equals the same handle with the term off and one static disc far
    away (both run the OBST kernels)"""
    p = params()
    B, ticks = 4, 20
    s0, seeds, paths = fleet_start(p, B, step=8)
    res = []
    for fleet in (False, True):
        bat = make(p, B, True, None if fleet else [far_discs(1)] * B, 50.0, paths, s0, seeds, fleet=(0.3, 0.0, 4, 50.0) if fleet else None)
        run = []
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            run.append(bits(bat))
        assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT
        if fleet:
            ns, nt, xyr = bat.resident_read_fleet()
            assert not ns.any() and not nt.any() and not xyr.any()
        res.append(run)
        bat.close()
    assert res[0] == res[1]


# 3. _read_fleet against the reference over the edge shapes -----------------------------------------------------------------------
def test_lists_of_300_robots_equal_the_reference():
    """B = 300 (the strided loop), K = 64, H = 10, start poses on a 0.25 m grid (exact ties), max_neighbours = 4 under a range
    that holds 20 grid neighbours (the cap), n_static dealt from {0, 30, 32} (M_y = 4, 2, 0): rows, counts and order of every tick
    equal the reference on the poses read after the previous tick; a run that reads nothing in between ends on the same lists."""
    p = params("diff_drive", 64, 10)
    B, ticks, maxn, rng = 300, 20, 4, 0.6
    px, py = BS.path_of(0)
    s0 = np.zeros((B, p.nstate))
    s0[:, 0] = 1.0 + 0.25 * (np.arange(B) % 20)      # (dyadic: the grid's distances are exact)
    s0[:, 1] = 0.25 * (np.arange(B) // 20) - 1.75
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)
    n_static = np.array([0, 30, 0, 32, 0, 0, 30] * 43, dtype=np.int32)[:B]
    static = [far_discs(int(n), b) for b, n in enumerate(n_static)]
    radius = 0.1 + 0.001 * np.arange(B)
    last = None
    for reading in (True, False):
        bat = make(p, B, True, static, 20.0, (px, py), s0, seeds, fleet=(radius, rng, maxn, 20.0))
        q = s0[:, :2].copy()
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if reading:
                ns, nt, xyr = bat.resident_read_fleet()
                n_total, rows = FR.lists(q, radius, n_static, maxn, rng)
                if it == 0:
                    taken = n_total - n_static
                    assert sorted(set(taken.tolist())) == [0, 2, 4]                 # (the cap and the full lists are exercised)
                    d2 = np.sum((rows[21][:, :2] - q[21]) ** 2, axis=1)
                    assert n_static[21] == 0 and d2.tolist() == [0.0625] * 4        # (robot 21's four rows: exact ties)
                np.testing.assert_array_equal(ns, n_static)
                np.testing.assert_array_equal(nt, n_total, err_msg="tick %d" % it)
                assert xyr.tobytes() == FR.table(static, rows).tobytes(), it
                q = bat.resident_read()[0][:, :2]
        fin = bat.resident_read_fleet()
        if last is not None:
            for a, b in zip(last, fin):
                assert a.tobytes() == b.tobytes()
        last = fin
        bat.close()


# 4. independence and restoration -------------------------------------------------------------------------------------------------
def test_a_robot_out_of_range_changes_no_bit_of_lists_without_it():
    """Robots 0 and 1 drive 3.7 m behind robots 2, 3 and 4 (range 1.5 m).  Moving robot 4's start 30 m away changes no bit, on
    any tick, of the robots whose lists held neither robot 4 nor, link by link, a robot whose list did (a neighbour that sees
    robot 4 drives differently, and its disc moves with it); it does change robots 2 and 3, which see robot 4."""
    p = params()
    B, ticks = 5, 10
    px, py = BS.path_of(0)
    s0, seeds, paths = fleet_start(p, B)
    for b, i in enumerate((5, 8, 45, 48, 51)):
        s0[b, 0], s0[b, 1] = px[i], py[i] + 0.05 * ((b % 5) - 2)
        s0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i])
    runs = []
    for moved in (False, True):
        s = s0.copy()
        if moved:
            s[4, :2] += (0.0, 30.0)
        bat = make(p, B, True, None, 50.0, paths, s, seeds, fleet=(0.2, 1.5, 2, 50.0))
        per_tick, sees, q = [], np.zeros((B, B), dtype=bool), s[:, :2].copy()
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            ns, nt, xyr = bat.resident_read_fleet()
            for y in range(B):   # (a tick's rows carry the positions at its start)
                for j in range(B):
                    sees[y, j] |= bool(np.any(np.all(xyr[y, :nt[y], :2] == q[j], axis=1)))
            per_tick.append([robot_bits(bat, b) for b in range(B)])
            q = bat.resident_read()[0][:, :2]
        runs.append((per_tick, sees.copy()))
        bat.close()
    sees = runs[0][1]
    touched = {4}
    while True:
        more = {y for y in range(B) if any(sees[y, j] for j in touched)} - touched
        if not more:
            break
        touched |= more
    assert touched == {2, 3, 4} and not runs[1][1][:4, 4].any()   # (the inputs' condition; moved away, robot 4 is in no list)
    for y in (0, 1):
        assert [t[y] for t in runs[0][0]] == [t[y] for t in runs[1][0]], y
    for y in (2, 3):
        assert [t[y] for t in runs[0][0]] != [t[y] for t in runs[1][0]], y


def test_turning_the_term_off_restores_kernel_and_bits():
    p = params()
    B, ticks = 5, 6
    s0, seeds, paths = fleet_start(p, B)

    def run(bat):
        bat.resident_set_poses(s0, seeds)
        bat.set_nominal(np.zeros((B, p.horizon - 1, p.udim)))
        out = []
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            out.append(bits(bat))
        return out, bat.last_kernel()

    bat = make(p, B, True, None, 0.0, paths, s0, seeds)
    want, k0 = run(bat)
    assert k0 == capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_VARIED | SHIFT
    bat.resident_set_fleet(0.2, 1.5, 2, 50.0)
    on, k1 = run(bat)
    assert k1 == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT and on != want
    r, rng, m = bat.resident_get_fleet()
    assert r.tolist() == [0.2] * B and rng == 1.5 and m == 2 and bat.get_obstacles()[1].tolist() == [50.0] * B
    bat.resident_set_fleet(None)
    r, rng, m = bat.resident_get_fleet()
    assert not r.any() and rng == 0.0 and m == 0 and not bat.get_obstacles()[1].any()
    with pytest.raises(MPPIError) as ei:
        bat.resident_read_fleet()
    assert ei.value.code == capi.ERR_STATE
    again, k2 = run(bat)
    assert k2 == k0 and again == want
    bat.close()


def test_removing_the_static_discs_keeps_the_fleet_rows():
    p = params()
    B = 5
    s0, seeds, paths = fleet_start(p, B)
    static = [far_discs(2, b) for b in range(B)]
    radius = np.full(B, 0.2)
    bat = make(p, B, True, static, 7.0, paths, s0, seeds, fleet=(radius, 1.5, 2, 50.0))
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    ns, nt, xyr = bat.resident_read_fleet()
    n_total, rows = FR.lists(s0[:, :2], radius, [2] * B, 2, 1.5)
    assert ns.tolist() == [2] * B and nt.tolist() == n_total.tolist() == [4] * B and xyr.tobytes() == FR.table(static, rows).tobytes()
    bat.set_obstacles(None)
    got, w = bat.get_obstacles()
    assert all(g.shape == (0, 3) for g in got) and w.tolist() == [50.0] * B   # (the later of the two setters gave the weight)
    q = bat.resident_read()[0][:, :2]
    bat.resident_step_enqueue(p.dt, 1, advance=True)
    ns, nt, xyr = bat.resident_read_fleet()
    n_total, rows = FR.lists(q, radius, [0] * B, 2, 1.5)
    assert not ns.any() and nt.tolist() == n_total.tolist() == [2] * B
    assert xyr.tobytes() == FR.table([np.zeros((0, 3))] * B, rows).tobytes()
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | OV | SHIFT
    # _set_obstacles under the term changes the static rows and counts only; _set_params keeps discs and fleet
    bat.set_obstacles(static, 9.0)
    bat.set_params([p] * B)
    q = bat.resident_read()[0][:, :2]
    bat.resident_step_enqueue(p.dt, 2, advance=True)
    ns, nt, xyr = bat.resident_read_fleet()
    n_total, rows = FR.lists(q, radius, [2] * B, 2, 1.5)
    assert ns.tolist() == [2] * B and nt.tolist() == n_total.tolist() and xyr.tobytes() == FR.table(static, rows).tobytes()
    assert bat.get_obstacles()[1].tolist() == [9.0] * B and bat.resident_get_fleet()[2] == 2
    bat.close()


# 5. refusals change nothing ---------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """After EACH refused call the getters return what was set, and the next tick's bits and _read_fleet lists equal those of
    a twin that saw no refused call."""
    p = params()
    B = 5
    s0, seeds, paths = fleet_start(p, B)
    radius, weight = np.array([0.15, 0.2, 0.1, 0.25, 0.3]), np.full(B, 50.0)
    bats = [make(p, B, True, None, 0.0, paths, s0, seeds, fleet=(radius, 1.5, 2, weight)) for _ in range(2)]
    bat, lib = bats[0], bats[0].lib
    tick = [0]

    def unchanged():
        r, rng, m = bat.resident_get_fleet()
        assert r.tolist() == radius.tolist() and rng == 1.5 and m == 2 and bat.get_obstacles()[1].tolist() == weight.tolist()
        for b in bats:
            b.resident_step_enqueue(p.dt, tick[0], advance=tick[0] > 0)
        tick[0] += 1
        assert bits(bats[0]) == bits(bats[1]), tick[0]
        assert [a.tobytes() for a in bats[0].resident_read_fleet()] == [a.tobytes() for a in bats[1].resident_read_fleet()], tick[0]

    for _ in range(3):
        unchanged()

    def refused(r, rng, m, w, code=capi.ERR_INVALID_ARG):
        r = None if r is None else capi.dptr(np.ascontiguousarray(r, dtype=np.float64))
        w = None if w is None else capi.dptr(np.ascontiguousarray(w, dtype=np.float64))
        assert lib.ccv_mppi_batch_resident_set_fleet(bat._h, r, float(rng), int(m), w) == code
        unchanged()

    ok = np.full(B, 0.4)
    refused(None, 1.0, 2, ok)
    refused(ok, 1.0, 2, None)
    for bad in (-1.0, np.nan, np.inf):
        refused([0.4, bad, 0.4, 0.4, 0.4], 1.0, 2, ok)
        refused(ok, 1.0, 2, [1.0, 1.0, bad, 1.0, 1.0])
        refused(ok, bad, 2, ok)
    for m in (0, -1, 33):
        refused(ok, 1.0, m, ok)
    x = np.zeros((B, 5))
    h = np.zeros((B, p.horizon))
    sd = np.zeros(B, dtype=np.uint64)
    for call in (lambda: bat.iterate(x, p.dt, h, h, 0.0, sd, 0), lambda: bat.iterate_enqueue(x, p.dt, h, h, 0.0, sd, 0)):
        with pytest.raises(MPPIError) as ei:
            call()
        assert ei.value.code == capi.ERR_STATE
        unchanged()
    assert tick[0] == 3 + 14 + 2
    for b in bats:
        b.close()


def test_more_than_1024_instances_are_refused_at_set():
    p = params("diff_drive", 64, 10)
    B = 1025
    px, py = BS.path_of(0)
    s0 = np.zeros((B, p.nstate))
    s0[:, 0], s0[:, 1] = px[5] + 0.01 * np.arange(B), py[5]
    res = []
    for attempt in (False, True):
        bat = make(p, B, False, None, 0.0, (px, py), s0, 7)
        if attempt:
            with pytest.raises(MPPIError) as ei:
                bat.resident_set_fleet(0.1, 1.0, 2, 1.0)
            assert ei.value.code == capi.ERR_INVALID_ARG and bat.resident_get_fleet()[2] == 0
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        res.append((bat.get_nominal().tobytes(), bat.last_kernel()))
        bat.close()
    assert res[0] == res[1]
    bat = make(p, 1024, False, None, 0.0, (px, py), s0[:1024], 7, fleet=(0.1, 0.05, 2, 1.0))   # the largest admitted batch: one tick
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    ns, nt, xyr = bat.resident_read_fleet()
    n_total, rows = FR.lists(s0[:1024, :2], np.full(1024, 0.1), np.zeros(1024, dtype=np.int32), 2, 0.05)
    np.testing.assert_array_equal(nt, n_total)
    assert xyr.tobytes() == FR.table([np.zeros((0, 3))] * 1024, rows).tobytes() and n_total.max() == 2
    bat.close()


# 6. memory ------------------------------------------------------------------------------------------------------------------
def test_fleet_returns_all_device_memory():
    import torch
    p = params()
    B = 16
    s0, seeds, paths = fleet_start(p, B)

    def cycle():
        bat = make(p, B, True, None, 0.0, paths, s0, seeds, fleet=(0.2, 1.5, 4, 10.0))
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        bat.resident_step_enqueue(p.dt, 1, advance=True)
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
    bat = make(p, B, True, None, 0.0, paths, s0, seeds)
    bat.resident_step_enqueue(p.dt, 0, advance=False)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(200):
        bat.resident_set_fleet(0.2 if i % 2 == 0 else None, 1.5 if i % 2 == 0 else 0.0, 4 if i % 2 == 0 else 0, 10.0)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 2 * 2**20
    bat.close()


# 7. behaviour ---------------------------------------------------------------------------------------------------------------
def test_two_robots_head_on_pass_at_a_larger_distance():
    """Two robots on the same straight 6 m path in opposite directions, 3 m apart at the start, shifted weights on, radii
    0.3 m + 0.3 m, range 3 m, weight 200, 90 ticks.  With the term off their closest approach (same tick) is below the 0.6 m of
    the two radii; with it on it is strictly larger than with it off.  (The figures are printed with -s)"""
    p = params()
    c = HEAD_ON
    B, ticks, paths, s0, seeds = 2, c["ticks"], c["paths"], c["s0"], c["seeds"]
    closest = []
    for on in (False, True):
        bat = make(p, B, True, None, 0.0, paths, s0, seeds, fleet=(c["radius"], c["range"], 1, c["weight"]) if on else None)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        t0, t1 = bat.resident_read_trace(0), bat.resident_read_trace(1)
        assert len(t0) == len(t1) == ticks
        closest.append(float(np.min(np.hypot(*(t0[:, :2] - t1[:, :2]).T))))
        bat.close()
    print("closest approach off / on: %.4f / %.4f" % tuple(closest))
    assert closest[0] < 0.6   # (the condition: with the term off the robots drive through one another)
    assert closest[1] > closest[0]

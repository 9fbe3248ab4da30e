"""GPU tests (-m gpu) that hold the fleet step's selection and its velocity rule at their edges on the device (fleet_step and
fleet_publish, csrc/mppi_fleet_device.h; DESIGN.md sections 10f and 10g), in all six prologue kernels.

The cases are tests/fleet_cases.py (pinned on the CPU by tests/test_fleet_reference.py), the reference is
tests/fleet_reference.py and, for the velocities, tests/fleet_velocity_reference.py; everything is compared as integers or
bytes.  Handles: diff drive, K = 64, H = 10 (fleet_support.make, static discs from fleet_support.far_discs).

Roads.  A read flushes, so the tick after a read runs the prologue kernel of its own (k_advance_batch_fleet[_pred]); a tick
enqueued straight after a tick runs inside the update launch (k_finalize_advance_batch[_shift]_fleet[_pred]).  Road "alone" is
set_poses, one tick, read; road "fused" is set_poses, two ticks that do not advance, read: the lists read are the fused
kernel's, formed on the same positions.  Every case runs on both roads for shifted weights off and on and prediction off and
on: the whole product, old cases and new (the file takes a few seconds on an MI355X).
"""
import numpy as np
import pytest

import batch_support as BS
import fleet_cases as FC
import fleet_reference as FR
import fleet_velocity_reference as FV
from ccv_mppi_path_tracker_amd import capi
from fleet_support import far_discs, fleet_start, make, params

pytestmark = pytest.mark.gpu

WEIGHT = 20.0
STATIC_V = (0.3, -0.2)    # the velocity of every static disc where a case has some (prediction leaves those rows the caller's)
COMBOS = [(False, False), (False, True), (True, False), (True, True)]   # (min_shift, prediction)
COMBO_IDS = ["%s-%s" % ("shift" if s else "plain_w", "pred" if v else "snap") for s, v in COMBOS]
BY_NAME = {c["name"]: c for c in FC.CASES}
_WANT = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def poses(p, q):
    s = np.zeros((len(q), p.nstate))
    s[:, :2] = q
    return s


def seeds_of(B):
    return np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)


def static_of(c):
    return [far_discs(int(n), b) for b, n in enumerate(c["n_static"])]


def want(c, step=0):
    """(n_total, disc table, velocity table of a first tick) of a case's position set by the reference, computed once"""
    key = (c["name"], step)
    if key not in _WANT:
        static = static_of(c)
        n_total, rows = FR.lists(*FC.args(c, FC.positions(c)[step]))
        _WANT[key] = (n_total, FR.table(static, rows), FV.table([np.tile(STATIC_V, (len(d), 1)) for d in static]))
    return _WANT[key]


def handle(p, c, shift, pred):
    B = len(c["q"])
    static = static_of(c) if c["n_static"].any() else None
    bat = make(p, B, shift, static, WEIGHT, BS.path_of(0), poses(p, c["q"]), seeds_of(B),
               fleet=(c["radius"], c["rng"], c["maxn"], WEIGHT))
    if pred:
        if static is not None:
            bat.set_obstacle_velocities([np.tile(STATIC_V, (len(d), 1)) for d in static])
        bat.resident_set_fleet_prediction(True)
    return bat


def check_lists(bat, c, step, pred, what):
    n_total, table, vtable = want(c, step)
    ns, nt, xyr = bat.resident_read_fleet()
    np.testing.assert_array_equal(ns, c["n_static"], err_msg=what)
    np.testing.assert_array_equal(nt, n_total, err_msg=what)
    bad = [y for y in range(len(nt)) if xyr[y].tobytes() != table[y].tobytes()]
    assert not bad, (what, "robots whose rows differ", bad[:8], xyr[bad[0]][:6], table[bad[0]][:6])
    if pred:   # a first tick, or the tick after one that did not advance: the static rows and zeros
        assert bat.resident_read_fleet_velocities().tobytes() == vtable.tobytes(), what


def run_roads(bat, p, c, pred, what):
    """both roads on every position set of the case, on one handle"""
    B = len(c["q"])
    for step, q in enumerate(FC.positions(c)):
        for road, ticks in (("alone", 1), ("fused", 2)):
            bat.resident_set_poses(poses(p, q), seeds_of(B))
            for it in range(ticks):
                bat.resident_step_enqueue(p.dt, it, advance=False)
            check_lists(bat, c, step, pred, "%s set %d %s" % (what, step, road))


# 1. every case through the six kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift,pred", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("name", [c["name"] for c in FC.CASES])
def test_lists_of_every_case_equal_the_reference_on_both_roads(name, shift, pred):
    p = params("diff_drive", 64, 10)
    c = BY_NAME[name]
    bat = handle(p, c, shift, pred)
    run_roads(bat, p, c, pred, name)
    assert bat.last_kernel() & capi.BATCH_KERNEL_OBST or bat.last_kernel() & capi.BATCH_KERNEL_MOVING
    assert bool(bat.last_kernel() & capi.BATCH_KERNEL_SHIFT) == shift
    bat.close()


@pytest.mark.parametrize("name", ["ties_m2", "on_range", "grid_m0_1_2"])
def test_lists_equal_the_reference_under_the_full_body_model(name):
    """fleet_step does not look at the model: one parametrisation of the second prologue form (five-state poses) is enough"""
    p = params("full_body", 64, 10)
    c = BY_NAME[name]
    bat = handle(p, c, True, True)
    run_roads(bat, p, c, True, name + " full_body")
    bat.close()


# 2. a list that shrinks leaves no row behind -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shift,pred", COMBOS, ids=COMBO_IDS)
def test_a_shrinking_list_leaves_no_stale_row_in_the_rollout(shift, pred):
    """`shrinking` on one handle: four neighbours each, then one each.  _read_fleet zeroes rows past the count on the host, so
    what shows that the rollout reads no row of the first set is a twin: the fleet term off, fed the second set's lists through
    set_obstacles, with the same warm start and seeds -- read_costs of every instance equal byte for byte, on both roads.  A
    second twin that is also given the rows the first set left behind must differ (the test can see a stale row)."""
    p = params("diff_drive", 64, 10)
    c = BY_NAME["shrinking"]
    B, seeds, static = len(c["q"]), seeds_of(len(c["q"])), static_of(c)
    s1 = poses(p, c["q_next"])
    zero_u = np.zeros((B, p.horizon - 1, p.udim))
    n0, rows0 = FR.lists(*FC.args(c))
    n1, rows1 = FR.lists(*FC.args(c, c["q_next"]))
    assert ((n0 - c["n_static"]) == 4).all() and ((n1 - c["n_static"]) == 1).all()
    clean = FR.full_lists(static, rows1)
    stale = [np.concatenate([d, r0[1:]]) for d, r0 in zip(clean, rows0)]     # rows 1 .. 3 of the first set still behind the count

    def costs(bat, ticks):
        bat.resident_set_poses(s1, seeds)
        bat.set_nominal(zero_u)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=False)
        return [bat.read_costs(b).tobytes() for b in range(B)]

    bat = handle(p, c, shift, pred)
    run_roads(bat, p, c, pred, "shrinking")
    got = {ticks: costs(bat, ticks) for ticks in (1, 2)}
    check_lists(bat, c, 1, pred, "shrinking, after the costs")
    bat.close()
    for lists, equal in ((clean, True), (stale, False)):
        twin = make(p, B, shift, None, WEIGHT, BS.path_of(0), s1, seeds)
        vels = [np.concatenate([np.tile(STATIC_V, (len(s), 1)), np.zeros((len(d) - len(s), 2))]) for s, d in zip(static, lists)]
        twin.set_obstacles(lists, WEIGHT, velocities=vels if pred else None)   # (a neighbour's velocity on a first tick: zero)
        for ticks in (1, 2):
            tw = costs(twin, ticks)
            if equal:
                assert [b for b in range(B) if tw[b] != got[ticks][b]] == [], ticks
            else:
                assert tw != got[ticks], ticks
        twin.close()


# 3. the velocity rule on the device ---------------------------------------------------------------------------------------------
def velocity_fleets(p):
    s0, seeds, _ = fleet_start(p, 5)
    static = [np.zeros((0, 3)), far_discs(3), np.zeros((0, 3)), far_discs(31, 1), np.zeros((0, 3))]
    five = dict(s0=s0, seeds=seeds, static=static, radius=np.array([0.15, 0.2, 0.1, 0.25, 0.3]), rng=1.5, maxn=2, odd=[])
    c = BY_NAME["not_finite_huge"]
    B = len(c["q"])
    odd = dict(s0=poses(p, c["q"]), seeds=seeds_of(B), static=[np.zeros((0, 3))] * B, radius=c["radius"], rng=c["rng"], maxn=c["maxn"],
               odd=list(range(6, B)))
    return dict(five=five, not_finite=odd)


STEPS = [("p.dt", True), (0.105, True), ("p.dt", False), (0.0, True), (1e-310, True), (5e-324, True)]


@pytest.mark.parametrize("road", ["alone", "fused", "fused_twice"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("fleet", ["five", "not_finite"])
def test_velocity_rows_equal_the_rule_at_every_dt(fleet, shift, road):
    """Prediction on.  For every (dt, advance): a tick that does not advance (it leaves a warm start that moves the robots), read
    q0, a tick with (dt, advance) -- fleet_publish forms the velocities --, on road "alone" read q1, then a tick (p.dt, no
    advance) -- fleet_step puts them beside the rows --, read q1 and the velocity table: it equals the rule on q0, q1 and dt
    beside the reference's selection on q1.  Road "fused" does not read between the last two ticks (the selection runs inside
    the update launch); road "fused_twice" does not read q0 either (it is the pose that was set: the first tick does not
    advance), so the velocities too are formed inside the update launch."""
    p = params("diff_drive", 64, 10)
    f = velocity_fleets(p)[fleet]
    B = len(f["s0"])
    n_static = np.array([len(d) for d in f["static"]], dtype=np.int32)
    static_v = [np.tile(STATIC_V, (len(d), 1)) for d in f["static"]]
    sv = FV.table(static_v)
    has_static = bool(n_static.any())
    bat = make(p, B, shift, f["static"] if has_static else None, WEIGHT, BS.path_of(0), f["s0"], f["seeds"],
               fleet=(f["radius"], f["rng"], f["maxn"], WEIGHT))
    if has_static:
        bat.set_obstacle_velocities(static_v)
    bat.resident_set_fleet_prediction(True)
    for dt, advance in STEPS:
        dt = p.dt if dt == "p.dt" else dt
        what = "%s dt=%r advance=%s" % (road, dt, advance)
        bat.resident_set_poses(f["s0"], f["seeds"])
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        q0 = f["s0"][:, :2] if road == "fused_twice" else bat.resident_read()[0][:, :2]
        assert q0.tobytes() == f["s0"][:, :2].tobytes(), what
        bat.resident_step_enqueue(dt, 1, advance=advance)
        if road == "alone":
            q1 = bat.resident_read()[0][:, :2]
        bat.resident_step_enqueue(p.dt, 2, advance=False)
        q_last = bat.resident_read()[0][:, :2]
        if road == "alone":
            assert q_last.tobytes() == q1.tobytes(), what
        q1 = q_last
        v = FV.velocity(q0, q1, dt, advance)
        n_total, rows, taken = FV.lists(q1, f["radius"], n_static, f["maxn"], f["rng"])
        expect = FV.table(FV.velocity_rows(static_v, taken, v))
        ns, nt, xyr = bat.resident_read_fleet()
        np.testing.assert_array_equal(nt, n_total, err_msg=what)
        assert xyr.tobytes() == FR.table(f["static"], rows).tobytes(), what
        got = bat.resident_read_fleet_velocities()
        print(what, "rows that are not zero beside the static ones:", int(np.any(got != sv, axis=2).sum()))
        assert got.tobytes() == expect.tobytes(), (what, got[0, :4], expect[0, :4])
        # the inputs' conditions
        if advance and dt in (p.dt, 0.105):
            assert (expect != sv).any() and (q1 != q0).any(), what            # robots that moved: a row that is not zero
        else:
            assert expect.tobytes() == sv.tobytes(), what                     # no advance, dt = 0, or 1 / dt = inf: zeros
        if dt in (1e-310, 5e-324):
            with np.errstate(over="ignore"):
                assert np.float64(1.0) / np.float64(dt) == np.inf
        # a position that is not finite: both components zero together (one finite component beside one that is not is held on
        # the CPU, tests/test_moving_obstacle_reference.py: here a robot at infinity or at NaN has no finite difference, and
        # one at +-1e200 does not move by a step)
        assert not v[f["odd"]].any(), what
        if not advance:   # ... and the robots at infinity and at +-1e200 stand in lists, their rows zero
            assert all(any(y in t.tolist() for t in taken) for y in f["odd"] if not np.isnan(q1[y]).any()), what
            assert len(f["odd"]) in (0, 6) and max(len(t) for t in taken) == (9 if f["odd"] else 2), what
    assert bat.last_kernel() & capi.BATCH_KERNEL_MOVING
    bat.close()

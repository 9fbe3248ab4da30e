"""GPU tests (-m gpu): rollout and cost over the whole heading range, against the extended-precision reference of
tests/rollout_reference.py and its derived rounding bound (pinned on the CPU by tests/test_rollout_reference.py).

Start headings (rollout_reference.headings()): 0.3; +-pi/4 with two neighbouring doubles on each side (the tie of the
reduction's rint); +-pi/2, +-3pi/4, +-pi and the double above pi; +-2.5, 100, -1234.5, +-9e4; the four doubles nearest above
a multiple of pi/2 (n <= 63 661); and per case theta_edge, the largest start heading fast_trig_safe (ccv_mppi_capi.hip) still
admits to the branch-free sin / cos, with the next double, which takes the plain kernel (a single handle does not expose its
launch plan: the results are asserted on both sides; the batch handle's last_kernel() is asserted).  The window is the
oracle's, turned about the start pose by the heading, yaw_ref0 = heading - 0.1: the robot is on its path at every heading
and no (sample, step) is at the 100 m gate (asserted as a condition).

Per case two fused iterations (the second from the first's u*): read_controls() equals the oracle's philox controls bit for
bit, read_candidates() is within bound_xy and read_costs() within bound_cost of the reference evaluated on those controls,
with T = T_MAX; T as measured from step 0 (measured_trig_ulps) is <= T_MAX.

Measured on an MI355X: T = 1 for every kernel family (default, r3, solo, v1) from the origin, where x_1 carries two roundings
besides the cosine, and T = 1 in every other case; the largest error is 0.81 of bound_xy (diff drive, the plain kernel) and
0.29 of bound_cost (full body, the plain kernel); the cooperative kernels stay below 0.76 / 0.26.
"""
import math

import numpy as np
import pytest

import helpers
import resident_loops as RL
import rollout_reference as RR
import ccv_mppi_path_tracker_amd as amd
from ccv_mppi_path_tracker_amd import BatchController, capi
from ccv_mppi_path_tracker_amd.controller import MPPIController

pytestmark = pytest.mark.gpu

T = RR.T_MAX
LD = np.longdouble
FAMILIES = {"diff_drive": (None, "r3", "solo", "v1"), "steering_diff_drive": (None, "r3", "solo", "v1"),
            "full_body": (None, "pc", "solo", "v1")}
CASES = [(model, fam, H, dt, variant) for model, H, dt, variant in RR.input_sets() for fam in FAMILIES[model]]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def check(r, controls_o, controls, cand, costs, what):
    """the per-case assertions; returns (error / bound of the positions, of the costs, measured T)"""
    assert not r.at_gate(), what
    if controls is not None:
        np.testing.assert_array_equal(controls, controls_o, err_msg=str(what))
    exy, ec, tm = r.err_xy_over_bound(cand, T), r.err_cost_over_bound(costs, T), RR.measured_trig_ulps(r, cand)
    print("%s: xy %.3f cost %.3f of the bound, T = %d" % (what, exy, ec, tm))
    assert exy <= 1.0, (what, exy)
    assert ec <= 1.0, (what, ec)
    assert tm <= RR.T_MAX, (what, tm)
    return exy, ec, tm


def run_case(g, o, p, variant, theta, iterations=2, origin=False):
    state, xr, yr, yaw0 = RR.case_inputs(p, variant, theta)
    if origin:
        xr, yr, state = xr - state[0], yr - state[1], np.concatenate([[0.0, 0.0], state[2:]])
    zero = np.zeros((p.horizon - 1, p.udim))
    g.set_nominal(zero)
    o.set_nominal(zero)
    worst = (0.0, 0.0, 1)
    for it in range(iterations):
        o.sampling(RR.SEED, rng="philox", iteration=it)
        u_g = g.iterate(state, p.dt, xr, yr, yaw0, RR.SEED, it, want_stats=False)
        u = o.get_controls()
        r = RR.reference(p, u, state, p.dt, xr, yr, yaw0)
        res = check(r, u, g.read_controls(), g.read_candidates(), g.read_costs(), (p.model, variant, theta, it))
        worst = tuple(max(a, b) for a, b in zip(worst, res))
        o.set_nominal(u_g)
    return worst


@pytest.mark.parametrize("model,family,H,dt,variant", CASES)
def test_rollout_and_cost_over_the_heading_range(monkeypatch, model, family, H, dt, variant):
    if family:
        monkeypatch.setenv("CCV_MPPI_KERNEL", family)
    p = RR.params_of(model, H, dt, variant)
    g, o = MPPIController(p), helpers.oracle_for(p)
    worst = (0.0, 0.0, 1)
    for theta in RR.case_headings(p, variant):
        worst = tuple(max(a, b) for a, b in zip(worst, run_case(g, o, p, variant, theta)))
    print("worst: xy %.3f cost %.3f of the bound, T = %d" % worst)
    g.close()


@pytest.mark.parametrize("family", [None, "r3", "solo", "v1"])
def test_trig_ulps_measured_from_the_origin(monkeypatch, family):
    """Diff drive from (0, 0): x_1 = v_0 cos(theta) dt carries two roundings besides the cosine, so T is measured sharply."""
    if family:
        monkeypatch.setenv("CCV_MPPI_KERNEL", family)
    p = RR.params_of("diff_drive", 9, 0.1)
    g, o = MPPIController(p), helpers.oracle_for(p)
    tm = max(run_case(g, o, p, None, theta, iterations=1, origin=True)[2] for theta in RR.case_headings(p, None))
    print("measured T = %d" % tm)
    assert tm <= RR.T_MAX
    g.close()


@pytest.mark.parametrize("model,variant", [("diff_drive", None), ("steering_diff_drive", None), ("full_body", "rp1")])
def test_stagewise_path_heading_west_south_west(model, variant):
    p = RR.params_of(model, 17, 0.1, variant)
    theta = -3 * math.pi / 4
    state, xr, yr, yaw0 = RR.case_inputs(p, variant, theta)
    g, o = MPPIController(p), helpers.oracle_for(p)
    o.sampling(RR.SEED, rng="philox", iteration=0)
    u = o.get_controls()
    g.inject_controls(u)
    g.predict_States(state, p.dt)
    g.calc_Weights(xr, yr, yaw0)
    r = RR.reference(p, u, state, p.dt, xr, yr, yaw0)
    check(r, u, g.read_controls(), g.read_candidates(), g.read_costs(), (model, "stage-wise", theta))
    g.close()


# ---- batch: every instance its own heading, the worst one decides the kernel --------------------------------------------------
def batch_headings(p, variant, B):
    edge, above = RR.edge_headings(p, p.dt, *(RR.ROLL_PITCH[variant] if variant else (0.0, 0.0)))
    hs = RR.headings()
    pick = [-3 * math.pi / 4, 9.0e4, hs[24], -math.pi, float(np.nextafter(math.pi / 4, 1.0)), -1234.5, 2.5, -9.0e4][:B - 1]
    return pick + [edge], above


def per_instance_params(p, B):
    out = []
    for b in range(B):
        lo, hi = list(p.u_min), list(p.u_max)
        lo[0], hi[0] = lo[0] * (1.0 - 0.05 * (b % 3)), hi[0] * (1.0 + 0.04 * (b % 4))
        out.append(p.with_(control_noise=0.5 + 0.03 * b, lam=1.0 + 0.1 * b, v_ref=p.v_ref + 0.02 * b, path_weight=1.0 + 0.5 * b,
                           v_weight=1.0 + 0.25 * (b % 2), u_min=tuple(lo), u_max=tuple(hi)))
    return out


@pytest.mark.parametrize("model,variant,B", [("diff_drive", None, 8), ("full_body", "rp1", 3)])
@pytest.mark.parametrize("varied", [False, True], ids=["shared", "per_instance"])
def test_batch_every_instance_its_own_heading(model, variant, B, varied):
    p = RR.params_of(model, 17, 0.1, variant)
    plist = per_instance_params(p, B) if varied else [p] * B
    thetas, above = batch_headings(p, variant, B)
    seeds = np.array([RR.SEED + 1000 * b for b in range(B)], dtype=np.uint64)
    bat = BatchController(plist if varied else p, B)
    for last in (thetas[-1], above):          # (theta_edge: the cooperative kernel; the next double: the plain one, for all)
        hs = thetas[:-1] + [last]
        inp = [RR.case_inputs(p, variant, th) for th in hs]
        x0 = np.array([i[0] for i in inp])
        xr, yr, yaw0 = np.array([i[1] for i in inp]), np.array([i[2] for i in inp]), np.array([i[3] for i in inp])
        nom = np.zeros((B, p.horizon - 1, p.udim))
        bat.set_nominal(nom)
        for it in range(2):
            u_b = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, it, want_stats=False)
            plain = (bat.last_kernel() & 0xF) == capi.BATCH_KERNEL_PLAIN
            assert plain == (last == above)
            for b in range(B):
                o = helpers.oracle_for(plist[b])
                o.set_nominal(nom[b])
                o.sampling(int(seeds[b]), rng="philox", iteration=it)
                u = o.get_controls()
                r = RR.reference(plist[b], u, x0[b], p.dt, xr[b], yr[b], yaw0[b])
                check(r, u, None, bat.read_candidates(b), bat.read_costs(b), (model, "batch", b, hs[b], it))
            nom = u_b
    bat.close()


# ---- resident loops heading west ---------------------------------------------------------------------------------------------
def turned_path(yaw):
    px, py = amd.make_path("sinusoid")
    return RR.rotated_window(px, py, px[0], py[0], yaw)


def plant_reference(p, s0, us):
    """the longdouble plant driven by the loop's own commands u*[0]: one sample, one step per tick"""
    u = np.array([uu[0] for uu in us[:-1]])[None, :, :]
    H = u.shape[1] + 1
    return RR.reference(p.with_(horizon=H), u, s0, p.dt, np.zeros(H), np.zeros(H), 0.0)


@pytest.mark.parametrize("yaw", [3.0, -3.0])
def test_resident_loop_heading_west(yaw):
    p = RR.params_of("diff_drive", 17, 0.1)
    px, py = turned_path(yaw)
    s0 = np.array([px[0], py[0], yaw])
    s0[:2] += 0.05 * np.array([-math.sin(yaw), math.cos(yaw)])
    ticks, seed = 12, 77
    poses, wins, us = RL.host_loop(p, px, py, s0, ticks, seed, p.num_samples)
    g = MPPIController(p)
    g.resident_set_path(px, py)
    g.resident_set_pose(s0)
    for it in range(ticks):
        g.resident_step_enqueue(p.dt, seed, it, advance=it > 0)
    st, idx, xr, yr, yaw0, steps = g.resident_read()
    assert steps == ticks and idx == wins[-1][0]
    np.testing.assert_array_equal(st, poses[-1])
    np.testing.assert_array_equal(xr, wins[-1][1])
    np.testing.assert_array_equal(yr, wins[-1][2])
    np.testing.assert_array_equal(g.get_nominal(), us[-1])
    np.testing.assert_array_equal(g.resident_read_trace()[:, :3], np.array(poses))
    r = plant_reference(p, s0, us)
    b = r.bound_xy(T)[0, -1]
    assert abs(float(LD(st[0]) - r.X[0, -1])) <= b and abs(float(LD(st[1]) - r.Y[0, -1])) <= b
    assert np.hypot(st[0] - s0[0], st[1] - s0[1]) > 0.3        # the loop drove along the path
    g.close()


@pytest.mark.parametrize("yaw", [3.0, -3.0])
def test_resident_batch_heading_west(yaw):
    p, B = RR.params_of("diff_drive", 17, 0.1), 3
    path = turned_path(yaw)
    s0 = np.array([[path[0][i], path[1][i], yaw + 0.05 * (b - 1)] for b, i in enumerate((0, 7, 15))])
    seeds = np.array([77, 78, 79], dtype=np.uint64)
    ticks = 12
    ref = RL.host_batch_loop(p, B, p.num_samples, s0, seeds, ticks, paths=[path] * B)
    bat = RL.resident_batch(p, B, p.num_samples, s0, seeds, paths=[path] * B)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
    st, idx, xr, yr, yaw0, steps = bat.resident_read()
    s, widx, wxr, wyr, wyaw0, u = ref[-1]
    assert steps == ticks
    np.testing.assert_array_equal(idx, widx)
    np.testing.assert_array_equal(st, s)
    np.testing.assert_array_equal(xr, wxr)
    np.testing.assert_array_equal(yr, wyr)
    np.testing.assert_array_equal(bat.get_nominal(), u)
    for b in range(B):
        r = plant_reference(p, s0[b], [row[5][b] for row in ref])
        bd = r.bound_xy(T)[0, -1]
        assert abs(float(LD(st[b, 0]) - r.X[0, -1])) <= bd and abs(float(LD(st[b, 1]) - r.Y[0, -1])) <= bd
    bat.close()


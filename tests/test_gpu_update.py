"""GPU tests (-m gpu) of the weighted update u* = sum w_k u_k / sum w_k where EVERY sample carries weight.

The parity tests run at the reference's lambda = 1, where one to thirty samples decide u* and a lost tail, a lost block or a
mis-paired sample cannot be seen (tests/test_update_reference.py pins that).  Here lambda is chosen from the case's own costs
(which do not depend on lambda: a first handle at lambda = 1 supplies them): flat, lambda = 1000, and graded,
lambda = (c_max - c_min) / ln 1000.  Every check feeds the device's OWN read-backs (costs, controls, weights) to the
extended-precision reference of tests/update_reference.py and asserts the derived rounding bound of an fp64 sum of K
products in any order -- u*, sum_w, every weight, min / max cost and the zero-weight count exactly, sum of the normalised
weights within K u of 1 -- and, as conditions on the INPUTS from K = 64 up, that losing any one sample would move u* by
>= 100 bounds and that pairing a sample's weight with its neighbour's controls would for >= 99 % of the pairs.

Which test reaches what (all but K = 1 with the sensitivity conditions asserted):
  four-wave / three-wave / two-wave / one-wave / plain kernel families ........ test_fused_iteration (kernel column)
  epilogue rows from LDS (H <= 17) and re-read from memory (H >= 25) ........... test_fused_iteration (H column)
  masked partial time block (H = 15, 80), one-step tail (H = 50) ............... test_fused_iteration
  ragged last workgroup (K = 65, 130, 1000, 4097), K = 1, 2, 63 ................ test_fused_iteration
  wide-turn instantiation, both clamp forms, no state store, steer_off ......... test_fused_iteration_options
  k_update_partials double2 body and scalar tail + k_finalize .................. test_stagewise_update_with_injected_controls
  MIN_SHIFT (k_min_cost, k_reweight, unfused update), single winner ............ test_min_shift, test_min_shift_where_plain_weights_underflow
  partial vector [S, V], shards with a ragged cut, deferred / immediate apply .. test_partials_and_sharded_apply
  k_finalize_exchange, rank-ordered sum ........................................ test_direct_exchange_two_ranks
  k_finalize_batch, both partial layouts; per-instance lambda .................. test_batch_update
  k_finalize_advance_batch (shared and varied) ................................. test_batch_resident_tick_pair
  one full pass of lane_partial_sum2 (1024 partials), two and eight passes ..... test_full_size_flat

The observed maxima of err / bound are printed per test (-s) and tabled in DESIGN.md; they are information: the assertion
is the bound.
"""
import math

import numpy as np
import pytest

import helpers
import update_reference as R
import ccv_mppi_path_tracker_amd as amd
from batch_support import MODEL_DEFAULTS, instance_seed
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController
from update_checks import batch_inputs, check_handle, check_update, host_controls, lambdas_for, report, set_kernel

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEED = 42


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def setup(wl, K, H, **over):
    """(params, state 0.05 m beside the path's start, window)"""
    w = configs.workload(wl, num_samples=K, horizon=H)
    p = w.params.with_(**over) if over else w.params
    path = helpers.oracle_path(w.path)
    state = np.zeros(p.nstate)
    state[0], state[1] = path[0][0], path[1][0] + 0.05
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    return p, state, xr, yr, yaw[0]


def regimes_for(K):
    return ("flat", "graded") if K >= 64 else ("flat",)


def probe_costs(p, state, xr, yr, yaw0, it, **kw):
    g = MPPIController(p.with_(lam=1.0), **kw)
    g.iterate(state, p.dt, xr, yr, yaw0, SEED, it, want_stats=False)
    c = g.read_costs()
    g.close()
    return c


def fused_case(monkeypatch, group, kernel, wl, K, H, over=None, handle_kw=None, env=None):
    set_kernel(monkeypatch, kernel)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    handle_kw = handle_kw or {}
    p, state, xr, yr, yaw0 = setup(wl, K, H, **(over or {}))
    c0 = probe_costs(p, state, xr, yr, yaw0, 7, **handle_kw)
    for regime in regimes_for(K):
        lam = R.regime_lambda(c0, regime)
        g = MPPIController(p.with_(lam=lam), **handle_kw)
        for it in (7, 8):    # (the second from the first one's update: the epilogue re-derives the controls from nominal_used)
            u, st = g.iterate(state, p.dt, xr, yr, yaw0, SEED, it)
            what = "%s %s K=%d H=%d %s it%d" % (kernel or "default", wl, K, H, regime, it)
            check_handle(group, what, g, lam, u, st)
            np.testing.assert_array_equal(g.get_nominal(), u)
            if K == 1:
                ctl = g.read_controls()[0]
                assert np.all(np.abs(u - ctl) <= 2 * np.spacing(np.abs(ctl)))
                assert g.read_weights()[0] == 1.0
        g.close()
    return p


# 1. the fused iteration, every kernel family ----------------------------------------------------------------------------
# H - 1 steps in time blocks of 8: 3, 9, 15, 17 -> at most two blocks (rows from LDS); 25, 50, 80, 128 -> re-read from memory;
# 15 and 80 end in a masked partial block, 50 in a one-step tail.  (r3 is built for diff drive and steering only.)
FUSED = [
    (None, "C2", 4097, 17), (None, "C2", 1000, 50), (None, "C3", 1000, 15), (None, "C3", 130, 25), (None, "C4", 130, 9),
    (None, "C4", 1000, 80), (None, "C2", 1, 17), (None, "C4", 1, 9), (None, "C2", 2, 3), (None, "C3", 63, 15),
    (None, "C2", 64, 128), (None, "C2", 65, 50),
    ("r4", "C2", 130, 9), ("r4", "C3", 1000, 50), ("r4", "C4", 65, 80), ("r4", "C3", 1, 15), ("r4", "C4", 4097, 17),
    ("r3", "C2", 130, 15), ("r3", "C3", 1000, 128), ("r3", "C3", 65, 3), ("r3", "C2", 1, 9),
    ("pc", "C4", 130, 17), ("pc", "C4", 1000, 25), ("pc", "C2", 4097, 50), ("pc", "C2", 1, 3), ("pc", "C3", 63, 80),
    ("solo", "C4", 130, 15), ("solo", "C4", 2048, 80), ("solo", "C2", 65, 9), ("solo", "C3", 1000, 50), ("solo", "C4", 1, 17),
    ("v1", "C2", 130, 17), ("v1", "C3", 1000, 50), ("v1", "C4", 65, 80), ("v1", "C2", 1, 9),
]


@pytest.mark.parametrize("kernel,wl,K,H", FUSED)
def test_fused_iteration(monkeypatch, kernel, wl, K, H):
    fused_case(monkeypatch, "fused", kernel, wl, K, H)


OPTIONS = [
    ("wide_turn", None, "C2", 1000, 50, {"dt": 0.41}, {}, {}),
    ("wide_turn_one_wave", "solo", "C2", 130, 17, {"dt": 0.41}, {}, {}),
    ("fast_clamp", None, "C2", 1000, 50, {"control_noise": 1.5}, {}, {}),
    ("select_clamp", None, "C2", 1000, 50, {"control_noise": 1.5}, {}, {"CCV_MPPI_FAST_CLAMP": "0"}),
    ("select_clamp_fb", None, "C4", 130, 80, {"control_noise": 1.5}, {}, {"CCV_MPPI_FAST_CLAMP": "0"}),
    ("fast_clamp_lds", "pc", "C3", 130, 15, {"control_noise": 1.5}, {}, {}),
    ("no_state_store", None, "C2", 1000, 50, {}, {"no_state_store": True}, {}),
    ("no_state_store_lds", None, "C3", 130, 9, {}, {"no_state_store": True}, {}),
    ("steer_off", None, "C4", 130, 9, {"steer_off": True}, {}, {}),
    ("steer_off_one_wave", "solo", "C4", 1000, 25, {"steer_off": True}, {}, {}),
]


@pytest.mark.parametrize("name,kernel,wl,K,H,over,handle_kw,env", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_fused_iteration_options(monkeypatch, name, kernel, wl, K, H, over, handle_kw, env):
    """dt = 0.41 with w_max = 2 rad/s: the diff-drive wide-turn instantiation; sigma = 1.5: many controls on a bound (asserted),
    with the two-instruction clamp and with compare-and-select; no state store: another store count in the four-wave
    epilogue; steer_off: the zeroed control dimension, whose rows must come out as exactly 0."""
    monkeypatch.delenv("CCV_MPPI_FAST_CLAMP", raising=False)
    p = fused_case(monkeypatch, "fused options", kernel, wl, K, H, over, handle_kw, env)
    if "control_noise" in over or "steer_off" in over:
        _, state, xr, yr, yaw0 = setup(wl, K, H, **over)
        g = MPPIController(p.with_(lam=1000.0), **handle_kw)
        u = g.iterate(state, p.dt, xr, yr, yaw0, SEED, 7, want_stats=False)
        ctl = g.read_controls()
        if "steer_off" in over:
            assert np.all(ctl[..., 2] == 0) and np.all(u[:, 2] == 0) and np.any(ctl[..., 1] != 0)
        else:
            lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
            assert np.mean((ctl == lo) | (ctl == hi)) > 0.05
        g.close()


# 2. stage-wise update with injected controls -----------------------------------------------------------------------------
def weyl_controls(p, K):
    """u[k][t][d] = lo + (hi - lo) frac(k phi1 + t phi2 + d phi3): no two elements alike, all inside the bounds"""
    k, t, d = np.ogrid[0:K, 0:p.horizon - 1, 0:p.udim]
    f = np.mod(k * (math.sqrt(2) - 1) + t * (math.sqrt(3) - 1) + d * (math.sqrt(5) - 2), 1.0)
    lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
    return lo + (hi - lo) * f


@pytest.mark.parametrize("wl,K,H", [("C2", K, 17) for K in (1, 2, 3, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4097)] +
                         [("C3", 2049, 50), ("C4", 257, 9), ("C4", 4097, 15)])
def test_stagewise_update_with_injected_controls(wl, K, H):
    """inject_controls -> predict_States -> calc_Weights -> determine_OptimalSolution: k_update_partials (256 threads take two
    samples each, 2048 samples per chunk; the scalar tail on odd K) + k_finalize."""
    p, state, xr, yr, yaw0 = setup(wl, K, H)
    ctl = weyl_controls(p, K)
    c0 = None
    for regime in (None,) + regimes_for(K):
        lam = 1.0 if regime is None else R.regime_lambda(c0, regime)
        g = MPPIController(p.with_(lam=lam))
        g.inject_controls(ctl)
        g.predict_States(state, p.dt)
        g.calc_Weights(xr, yr, yaw0)
        u, st = g.determine_OptimalSolution(want_stats=True)
        if regime is None:
            c0 = g.read_costs()
        else:
            np.testing.assert_array_equal(g.read_controls(), ctl)
            check_handle("stage-wise", "%s K=%d H=%d %s" % (wl, K, H, regime), g, lam, u, st)
            if K == 1:
                assert np.all(np.abs(u - ctl[0]) <= 2 * np.spacing(np.abs(ctl[0]))) and g.read_weights()[0] == 1.0
        g.close()


# 3. MIN_SHIFT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [None, "v1"])
@pytest.mark.parametrize("wl,K,H", [("C2", 1000, 17), ("C4", 130, 9), ("C3", 2049, 50)])
def test_min_shift(monkeypatch, kernel, wl, K, H):
    """w = exp(-(c - min c) / lambda): k_min_cost + k_reweight + the unfused update, after the production rollout and after the
    plain one.  Flat, graded, and a single-winner lambda so small that the second-best shifted weight is below 2^-60: u* is the
    arg-min sample's controls within 2 ulp and sum_w is 1 within 1 ulp."""
    set_kernel(monkeypatch, kernel)
    p, state, xr, yr, yaw0 = setup(wl, K, H)
    c0 = probe_costs(p, state, xr, yr, yaw0, 7, min_shift=True)
    for regime in ("flat", "graded"):
        lam = R.regime_lambda(c0, regime)
        g = MPPIController(p.with_(lam=lam), min_shift=True)
        for it in (7, 8):
            u, st = g.iterate(state, p.dt, xr, yr, yaw0, SEED, it)
            check_handle("min_shift", "%s %s K=%d H=%d %s it%d" % (kernel or "default", wl, K, H, regime, it), g, lam, u, st,
                         shift=True)
        g.close()
    cs = np.sort(c0)
    lam = (cs[1] - cs[0]) / (64 * math.log(2.0))
    assert lam > 0
    g = MPPIController(p.with_(lam=lam), min_shift=True)
    u, st = g.iterate(state, p.dt, xr, yr, yaw0, SEED, 7)
    c = g.read_costs()
    np.testing.assert_array_equal(c, c0)
    best = g.read_controls()[int(np.argmin(c))]
    assert np.all(np.abs(u - best) <= 2 * np.spacing(np.abs(best)))
    assert abs(st.sum_w - 1.0) <= np.spacing(1.0)
    check_handle("min_shift", "%s %s K=%d single winner" % (kernel or "default", wl, K), g, lam, u, st, shift=True, sens=False)
    g.close()


def test_min_shift_where_plain_weights_underflow():
    """The case of test_all_weights_underflow_gives_nan_like_the_reference (far from the path, path_weight 1e4) in the graded
    regime: every unshifted weight is 0 (asserted), the shifted update is finite and within the bound."""
    p = configs.workload("C2").params.with_(num_samples=128, horizon=20, path_weight=1e4)
    path = helpers.oracle_path("sinusoid")
    state = np.array([3.0, 40.0, 0.0])
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    c0 = probe_costs(p, state, xr, yr, yaw[0], 0, min_shift=True)
    lam = R.regime_lambda(c0, "graded")
    assert np.all(np.exp(-c0 / lam) == 0.0)
    g = MPPIController(p.with_(lam=lam), min_shift=True)
    u, st = g.iterate(state, p.dt, xr, yr, yaw[0], SEED, 0)
    check_handle("min_shift", "underflow K=128 graded", g, lam, u, st, shift=True)
    g.close()


# 4. partials ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl,K,H", [("C2", 4097, 17), ("C4", 1000, 80), ("C3", 2049, 50)])
@pytest.mark.parametrize("regime", ["flat", "graded"])
def test_partials_and_sharded_apply(wl, K, H, regime):
    import torch
    p, state, xr, yr, yaw0 = setup(wl, K, H)
    lam = R.regime_lambda(probe_costs(p, state, xr, yr, yaw0, 7), regime)
    p = p.with_(lam=lam)
    cut = K // 2 + 1
    a, b = MPPIController(p, num_samples=cut), MPPIController(p, num_samples=K - cut, sample_offset=cut)
    n = a.partials_size()
    pa, pb = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    a.iterate_partials_enqueue(state, p.dt, xr, yr, yaw0, SEED, 7, pa.data_ptr())
    b.iterate_partials_enqueue(state, p.dt, xr, yr, yaw0, SEED, 7, pb.data_ptr())
    a.synchronize()
    b.synchronize()
    acc = R.Accumulator(lam)
    what = "%s K=%d H=%d %s" % (wl, K, H, regime)
    for g, vec in ((a, pa), (b, pb)):
        v = vec.cpu().numpy()
        c, ctl = g.read_costs(), g.read_controls()
        ref = R.reference(c, ctl, lam)
        assert abs(LD(v[0]) - ref.S) <= ref.bound_S()
        rv = np.max(np.abs(v[1:].astype(LD) - ref.V).astype(np.float64) / ref.bound_V())
        report("partials", what + " shard V", rv)
        assert rv <= 1.0
        acc.add(c, ctl)
    ca = np.concatenate([a.read_costs(), b.read_costs()])
    ua = np.concatenate([a.read_controls(), b.read_controls()])
    tot = pa + pb
    torch.cuda.synchronize()
    a.apply_partials_enqueue(tot.data_ptr())
    u_now = a.get_nominal()                       # performed at once
    b.apply_partials_enqueue(tot.data_ptr())      # deferred into the next launch, which divides while it stages the warm start
    b.iterate_partials_enqueue(state, p.dt, xr, yr, yaw0, SEED, 8, pb.data_ptr())
    b.synchronize()
    u_deferred = b.get_nominal()
    s = float(tot[0].item())
    check_update("partials", what + " apply at once", ca, ua, lam, u_now, s)
    check_update("partials", what + " deferred apply", ca, ua, lam, u_deferred, s, sens=False)
    a.close()
    b.close()


# 5. direct exchange ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl,K,H,regime", [("C2", 1001, 17, "flat"), ("C2", 1001, 17, "graded"), ("C3", 4097, 50, "graded")])
def test_direct_exchange_two_ranks(wl, K, H, regime):
    """Two handles of one process connected as ranks 0 and 1, both iterate: u* of both within the bound of the reference over
    the concatenated samples, and the same bits on both."""
    p, state, xr, yr, yaw0 = setup(wl, K, H)
    lam = R.regime_lambda(probe_costs(p, state, xr, yr, yaw0, 7), regime)
    p = p.with_(lam=lam)
    cut = K // 2 + 1
    c, d = MPPIController(p, num_samples=cut), MPPIController(p, num_samples=K - cut, sample_offset=cut)
    blobs = [c.exchange_create(2, 0), d.exchange_create(2, 1)]
    c.exchange_connect(blobs)
    d.exchange_connect(blobs)
    for it in (7, 8):
        c.iterate_exchange_enqueue(state, p.dt, xr, yr, yaw0, SEED, it)
        d.iterate_exchange_enqueue(state, p.dt, xr, yr, yaw0, SEED, it)
        uc, ud = c.get_nominal(), d.get_nominal()
        np.testing.assert_array_equal(uc, ud)
        costs = np.concatenate([c.read_costs(), d.read_costs()])
        ctl = np.concatenate([c.read_controls(), d.read_controls()])
        check_update("exchange", "%s K=%d H=%d %s it%d" % (wl, K, H, regime, it), costs, ctl, lam, uc)
    c.close()
    d.close()


# 6. batch handles ---------------------------------------------------------------------------------------------------------
def check_batch(group, what, bat, plist, kinds, noms, seeds, it, u, stats=None):
    for b, p in enumerate(plist):
        ctl = host_controls(p, noms[b], seeds[b], it)
        check_update(group, "%s b=%d %s" % (what, b, kinds[b]), bat.read_costs(b), ctl, p.lam, u[b],
                     stats[b].sum_w if stats else None, bat.read_weights(b), stats[b] if stats else None,
                     sens=kinds[b] != "one")


BATCH = [(None, "diff_drive", 1000, 15, 8), (None, "diff_drive", 63, 17, 3), (None, "steering_diff_drive", 1000, 50, 3),
         (None, "diff_drive", 1000, 15, 1), (None, "full_body", 1000, 15, 3), (None, "full_body", 10000, 15, 3),
         ("v1", "diff_drive", 1000, 15, 3), ("v1", "full_body", 63, 9, 8), ("v1", "steering_diff_drive", 1000, 25, 1)]


@pytest.mark.parametrize("varied", [False, True], ids=["shared", "varied"])
@pytest.mark.parametrize("kernel,model,K,H,B", BATCH)
def test_batch_update(monkeypatch, kernel, model, K, H, B, varied):
    """k_finalize_batch over the fused kernels' partial layout (four-wave; one-wave: full body, 3 x 157 workgroups) and over
    k_update_partials_batch's (CCV_MPPI_KERNEL=v1), shared and per-instance parameters, two iterations."""
    import torch
    set_kernel(monkeypatch, kernel)
    p = MODEL_DEFAULTS[model](K, H)
    x0, xr, yr, yaw0, seeds = batch_inputs(p, B)
    probe = BatchController(p, B)
    probe.iterate(x0, p.dt, xr, yr, yaw0, seeds, 7, want_stats=False)
    lk = lambdas_for([probe.read_costs(b) for b in range(B)], varied)
    probe.close()
    kinds = [k for k, _ in lk]
    plist = [p.with_(lam=l) for _, l in lk]
    bat = BatchController(plist, B) if varied else BatchController(plist[0], B)
    if not varied:
        plist = [plist[0]] * B     # (flat: lambda = 1000 whatever the costs)
    noms = np.zeros((B, H - 1, p.udim))
    for it in (7, 8):
        u, st = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, it)
        check_batch("batch", "%s %s K=%d B=%d it%d" % (kernel or "default", model, K, B, it), bat, plist, kinds, noms, seeds,
                    it, u, st)
        np.testing.assert_array_equal(bat.get_nominal(), u)
        noms = u
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblk = B * (-(-K // 64))
    fam = capi.BATCH_KERNEL_PLAIN if kernel == "v1" else (
        capi.BATCH_KERNEL_ONE_WAVE if nblk > (1 if model == "full_body" else 5) * cus else capi.BATCH_KERNEL_FOUR_WAVE)
    assert bat.last_kernel() & ~(capi.BATCH_KERNEL_VARIED | capi.BATCH_KERNEL_WIDE) == fam
    assert bool(bat.last_kernel() & capi.BATCH_KERNEL_VARIED) == varied
    bat.close()


@pytest.mark.parametrize("varied", [False, True], ids=["shared", "varied"])
@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 1000, 15, 3), ("steering_diff_drive", 1000, 17, 8)])
def test_batch_resident_tick_pair(model, K, H, B, varied):
    """Two resident ticks back to back: the first tick's update is launched with the second tick's prologue
    (k_finalize_advance_batch / _varied), and the second tick samples around what it wrote.  Batch X runs tick 0 alone and is
    read back (u0 through the flush: checked against tick 0's samples); batch Y runs both ticks without a read in between;
    its tick-1 costs, weights and u1 must fit the samples rebuilt around X's u0 -- a u0 off by more than rounding in Y's
    fused finalize shifts every tick-1 control and u1 with it, which is orders above the bound."""
    p = MODEL_DEFAULTS[model](K, H)
    paths = [amd.make_path("sinusoid" if b % 2 == 0 else "dkan") for b in range(B)]
    s0 = np.zeros((B, p.nstate))
    for b in range(B):
        i = 7 * b + 3
        s0[b, 0], s0[b, 1] = paths[b][0][i], paths[b][1][i] + 0.05
        s0[b, 2] = np.arctan2(paths[b][1][i + 1] - paths[b][1][i], paths[b][0][i + 1] - paths[b][0][i])
    seeds = np.array([instance_seed(b) for b in range(B)], dtype=np.uint64)

    def make(params):
        bat = BatchController(params, B)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        return bat

    probe = make(p)
    probe.resident_step_enqueue(p.dt, 0, advance=False)
    probe.synchronize()
    lk = lambdas_for([probe.read_costs(b) for b in range(B)], varied)
    probe.close()
    kinds = [k for k, _ in lk]
    plist = [p.with_(lam=l) for _, l in lk]
    params = plist if varied else plist[0]
    if not varied:
        plist = [plist[0]] * B
    X, Y = make(params), make(params)
    X.resident_step_enqueue(p.dt, 0, advance=False)
    u0 = X.get_nominal()
    what = "%s K=%d B=%d %s" % (model, K, B, "varied" if varied else "shared")
    check_batch("batch resident", what + " tick0 (flush)", X, plist, kinds, np.zeros((B, H - 1, p.udim)), seeds, 0, u0)
    Y.resident_step_enqueue(p.dt, 0, advance=False)
    Y.resident_step_enqueue(p.dt, 1, advance=True)
    u1 = Y.get_nominal()
    check_batch("batch resident", what + " tick1 (after the fused finalize)", Y, plist, kinds, u0, seeds, 1, u1)
    assert bool(Y.last_kernel() & capi.BATCH_KERNEL_VARIED) == varied
    X.close()
    Y.close()


# 7. full sizes, flat regime ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl,K,spread", [("C2", 65536, None), ("C3", 65536, None), ("C4", 131072, None), ("C5", 524288, 100.0)])
def test_full_size_flat(wl, K, spread):
    """One iteration at lambda = 1000 -- but for K = 524 288, whose inputs fail the conditions there: the bound grows with K
    while neighbouring weights differ by ~1/lambda, so 5.5 % of the pairs fall below 100 in the flat regime, and the graded
    one (ln 1000) leaves a drop sensitivity of 81 (CPU oracle, same inputs).  A case that fails gets another lambda, not a
    looser condition: (c_max - c_min) / ln 100 there (oracle: minimum drop sensitivity 693, 0.64 % of the pairs below 100),
    the costs taken from a first handle at lambda = 1 that is closed before the one under test is created.  The fused path has one partial per workgroup of 64 samples: 1024 at C2 / C3 (one full
    pass of lane_partial_sum2), 2048 at C4 and 8192 at K = 524 288 (two and eight passes).  The controls are read back in
    slices of at most 64 MB and S, V, A accumulated in extended precision; a second sweep takes the sensitivities."""
    w = configs.workload(wl)
    p = w.params
    assert p.num_samples == K
    path = helpers.oracle_path(w.path)
    state = np.zeros(p.nstate)
    state[0], state[1] = path[0][0], path[1][0] + 0.05
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    nominal = np.random.default_rng(1).normal(0, 0.2, size=(p.horizon - 1, p.udim))
    lam = 1000.0
    if spread:
        g = MPPIController(p.with_(lam=1.0))
        g.set_nominal(nominal)
        g.iterate(state, p.dt, xr, yr, yaw[0], SEED, 7, want_stats=False)
        c = g.read_costs()
        g.close()
        lam = float(c.max() - c.min()) / math.log(spread)
    p = p.with_(lam=lam)
    g = MPPIController(p)
    g.set_nominal(nominal)
    u, st = g.iterate(state, p.dt, xr, yr, yaw[0], SEED, 7)
    c, wn = g.read_costs(), g.read_weights()
    step = max(64, (64 * 2 ** 20 // (8 * (p.horizon - 1) * p.udim)) // 64 * 64)
    acc = R.Accumulator(lam)
    for first in range(0, K, step):
        n = min(step, K - first)
        acc.add(c[first:first + n], g.read_controls(first, n))
    ref = acc.finish()
    w_dev = wn * st.sum_w
    E = R.measured_exp_ulps(c, lam, w_dev)
    assert E <= R.E_MAX and R.check_weights(c, lam, w_dev, E) <= 1.0
    ratio = ref.err_over_bound(u, E)
    report("full size", "%s K=%d" % (wl, K), ratio)
    assert ratio <= 1.0
    assert abs(LD(st.sum_w) - ref.S) <= ref.bound_S(E)
    assert st.min_cost == c.min() and st.max_cost == c.max() and st.n_zero_weight == 0 and st.nonfinite == 0
    assert abs(math.fsum(wn) - 1.0) <= K * R.U
    lo, below, pairs = np.inf, 0, 0
    for first in range(0, K, step):
        n = min(step + 1, K - first)      # (one sample of overlap: the pair across the slice boundary)
        drop, swap = R.sensitivities(c[first:first + n], g.read_controls(first, n), ref, E)
        lo, below, pairs = min(lo, drop.min()), below + int((swap < 100.0).sum()), pairs + len(swap)
    print("full size %s: min drop sensitivity %.3g, pairs below 100: %.3f %%" % (wl, lo, 100.0 * below / pairs))
    assert lo >= 100.0 and below <= 0.01 * pairs
    g.close()

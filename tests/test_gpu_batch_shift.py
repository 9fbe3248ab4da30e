"""GPU tests (-m gpu) of the batch handles' shifted-weight mode (ccv_mppi_batch_set_min_shift, BatchController(min_shift=True)):
w = exp(-(c - min c) / lambda_b) per instance, formed inside the fused iteration as block-relative weights that the update
rescales (k_finalize_batch_shift), and by the exact shift behind the plain kernel (k_min_cost_batch, k_reweight_batch).

The bound.  Every check feeds the instance's OWN read-backs (costs, normalised weights; controls rebuilt on the host from the
seed and the warm start, as test_gpu_update.check_batch does) to update_reference.reference(costs, controls, lambda_b,
shift = min cost) and asserts update_reference's own formulas with E = E_SHIFT ulps per weight instead of the exp's E:

  * A device weight is a product of two exp results, w_k = exp(-fl(fl(c_k - m_g) / lambda)) * exp(-fl(fl(m_g - m) / lambda)),
    m_g the minimum of the sample's workgroup, m the instance's.  With x1 = (c_k - m_g) / lambda >= 0 and x2 = (m_g - m) /
    lambda >= 0 the rounded difference and the rounded quotient put at most 2 u x1 and 2 u x2 on the two arguments, and
    x1 + x2 = x = (c_k - m) / lambda exactly: together 2 u x, which is the factor 2 update_reference applies to X whenever a
    shift is given (UpdateRef.xmax, and k = 2 in its weight formulas).
  * Each exp is off by at most E_MAX ulps: (1 + E_MAX u)^2, i.e. 2 E_MAX ulps on the product of the exact exponentials.
  * One more rounding: in the sums the scale multiplies a workgroup's sum, s_g * (sum_k w_k u_k), one rounding that every
    product of the workgroup carries; in the read-back it is the rounding of w_k * s_g itself.  Either way one ulp per weight.

  E_SHIFT = 2 * E_MAX + 1 = 9.

With that E: u* within bound_u(E_SHIFT), sum_w within bound_S(E_SHIFT) (and >= 1), the zero-weight count within
zero_count_range(E_SHIFT), every weight (normalised weight times sum_w: + 2 roundings, as update_reference counts them) within
(2 |x| + E_SHIFT + 2) u w with the floor 2^-1074 (E_SHIFT + 1), min / max cost exact, the normalised weights' sum within K u
of 1, and the sensitivity conditions on the inputs (drop >= 100 for every sample, swap >= 100 for >= 99 % of the pairs) wherever
lambda comes from regime_lambda.  The plain family (exact shift, one exp) is held to the same E_SHIFT: it needs less.
The observed maxima of err / bound are printed (-s); the assertion is the bound.
"""
import numpy as np
import pytest

import batch_support as BS
import ccv_mppi_path_tracker_amd as amd
import helpers
import update_checks as UC
import update_reference as R
from batch_support import MODEL_DEFAULTS, SV
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIError
from update_checks import check_shift

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def check_batch_shift(what, bat, plist, kinds, noms, seeds, it, u, stats=None, only=None):
    for b, p in enumerate(plist):
        if only is not None and b not in only:
            continue
        ctl = UC.host_controls(p, noms[b], seeds[b], it)
        check_shift("%s b=%d %s" % (what, b, kinds[b]), bat.read_costs(b), ctl, p.lam, u[b],
                    stats[b].sum_w if stats else None, bat.read_weights(b), stats[b] if stats else None,
                    sens=kinds[b] != "one")


def family_code(kernel, model, K, B):
    if kernel == "v1":
        return capi.BATCH_KERNEL_PLAIN
    nblk = B * (-(-K // 64))
    return capi.BATCH_KERNEL_ONE_WAVE if nblk > (1 if model == "full_body" else 5) * BS.cus() else capi.BATCH_KERNEL_FOUR_WAVE


# 1. against the extended-precision reference ------------------------------------------------------------------------------
# four-wave: dd tail (H = 15), dd no tail (H = 50), dd wide (dt = 0.41), sd tail / no tail, fb tail / no tail; one-wave: dd, sd
# (13 x 100 workgroups: update_checks.batch_inputs has poses for 14 instances), fb (3 x 157); plain: dd, sd, fb;
# K = 65 537: 1025 workgroups per instance, the smallest count that takes the update's second pass over the partial columns
# (shift_scaled_sum2 and the statistics wave beyond 1024 columns), the last workgroup with one live sample
CASES = [(None, "diff_drive", 1000, 15, 8, {}), (None, "diff_drive", 1000, 50, 3, {}), (None, "diff_drive", 1000, 50, 3, {"dt": 0.41}),
         (None, "steering_diff_drive", 1000, 15, 3, {}), (None, "steering_diff_drive", 1000, 50, 3, {}),
         (None, "full_body", 1000, 15, 3, {}), (None, "full_body", 130, 9, 3, {}),
         (None, "diff_drive", 6400, 15, 13, {}), (None, "steering_diff_drive", 6400, 25, 13, {}), (None, "full_body", 10000, 15, 3, {}),
         (None, "diff_drive", 63, 17, 3, {}), (None, "diff_drive", 1000, 15, 1, {}),
         ("v1", "diff_drive", 1000, 15, 3, {}), ("v1", "steering_diff_drive", 1000, 25, 1, {}), ("v1", "full_body", 63, 9, 8, {}),
         (None, "diff_drive", 65537, 15, 2, {})]   # (last: the ids of the cases above carry their position)


@pytest.mark.parametrize("varied", [False, True], ids=["shared", "varied"])
@pytest.mark.parametrize("kernel,model,K,H,B,over", CASES)
def test_shifted_update_against_the_reference(monkeypatch, kernel, model, K, H, B, over, varied):
    UC.set_kernel(monkeypatch, kernel)
    p = MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**over)
    x0, xr, yr, yaw0, seeds = UC.batch_inputs(p, B)
    probe = BatchController(p, B)
    probe.iterate(x0, p.dt, xr, yr, yaw0, seeds, 7, want_stats=False)
    lk = UC.lambdas_for([probe.read_costs(b) for b in range(B)], varied)
    probe.close()
    kinds = [k for k, _ in lk]
    plist = [p.with_(lam=l) for _, l in lk]
    bat = BatchController(plist if varied else plist[0], B, min_shift=True)
    assert bat.get_min_shift()
    if not varied:
        plist = [plist[0]] * B
    noms = np.zeros((B, H - 1, p.udim))
    what = "%s %s K=%d H=%d B=%d %s" % (kernel or "default", model, K, H, B, "varied" if varied else "shared")
    for it in (7, 8):
        u, st = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, it)
        check_batch_shift(what + " it%d" % it, bat, plist, kinds, noms, seeds, it, u, st)
        np.testing.assert_array_equal(bat.get_nominal(), u)
        noms = u
    wide = capi.BATCH_KERNEL_WIDE if "dt" in over else 0
    assert bat.last_kernel() == SV | wide | family_code(kernel, model, K, B)
    bat.close()


def test_single_winner():
    """lambda so small that every cost but the smallest lies more than 1600 lambda above it: every other sample's weight is 0
    through its own factor or its workgroup's scale, u* is the arg-min sample's controls within 2 ulp, sum_w is exactly 1 and
    the zero-weight count is K - 1."""
    K, H, B = 1000, 15, 3
    p = configs.diff_drive_defaults(K, H)
    x0, xr, yr, yaw0, seeds = UC.batch_inputs(p, B)
    probe = BatchController(p, B)
    probe.iterate(x0, p.dt, xr, yr, yaw0, seeds, 7, want_stats=False)
    c0 = [probe.read_costs(b) for b in range(B)]
    probe.close()
    plist = []
    for c in c0:
        cs = np.sort(c)
        assert cs[1] > cs[0]
        plist.append(p.with_(lam=float(cs[1] - cs[0]) / 1600.0))
    bat = BatchController(plist, B, min_shift=True)
    u, st = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, 7)
    for b in range(B):
        c = bat.read_costs(b)
        np.testing.assert_array_equal(c, c0[b])
        best = UC.host_controls(plist[b], np.zeros((H - 1, p.udim)), seeds[b], 7)[int(np.argmin(c))]
        assert np.all(np.abs(u[b] - best) <= 2 * np.spacing(np.abs(best)))
        assert st[b].sum_w == 1.0 and st[b].n_zero_weight == K - 1 and st[b].nonfinite == 0
        w = bat.read_weights(b)
        assert w[int(np.argmin(c))] == 1.0 and np.count_nonzero(w) == 1
    bat.close()


# 2. where the plain weights underflow ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [None, "v1"])
def test_where_the_plain_weights_underflow(monkeypatch, kernel):
    """Odd instances start 40 m beside the path with path_weight 1e4 (the case of test_min_shift_where_plain_weights_underflow):
    in the graded regime their min cost / lambda is beyond 800 and every plain weight is 0; the even instances start on the
    path.  Shift off: the odd instances return NaN and sum_w == 0.  Shift on, same handle: every instance passes check 1."""
    UC.set_kernel(monkeypatch, kernel)
    B, K, H = 4, 1000, 20
    p = configs.workload("C2").params.with_(num_samples=K, horizon=H, path_weight=1e4)
    path = helpers.oracle_path("sinusoid")
    x0, xr, yr, yaw0 = np.zeros((B, 3)), np.zeros((B, H)), np.zeros((B, H)), np.zeros(B)
    for b in range(B):
        x0[b] = (3.0, 40.0, 0.0) if b % 2 else (path[0][5 * b], path[1][5 * b] + 0.05, 0.0)
        xr[b], yr[b], yaw = helpers.oracle_window(p, path, x0[b])
        yaw0[b] = yaw[0]
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)
    probe = BatchController(p, B)
    probe.iterate(x0, p.dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    c0 = [probe.read_costs(b) for b in range(B)]
    probe.close()
    plist = [p.with_(lam=R.regime_lambda(c, "graded")) for c in c0]
    for b in range(B):
        if b % 2:
            assert c0[b].min() / plist[b].lam > 800.0 and np.all(np.exp(-c0[b] / plist[b].lam) == 0.0)
        else:
            assert c0[b].min() / plist[b].lam < 700.0
    bat = BatchController(plist, B)
    u, st = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, 0)
    for b in range(B):
        if b % 2:
            assert np.all(np.isnan(u[b])) and st[b].sum_w == 0.0 and st[b].nonfinite == 1
        else:
            assert np.all(np.isfinite(u[b])) and st[b].sum_w > 0.0
    bat.set_min_shift(True)
    noms = np.zeros((B, H - 1, p.udim))
    bat.set_nominal(noms)
    u, st = bat.iterate(x0, p.dt, xr, yr, yaw0, seeds, 0)
    assert np.all(np.isfinite(u)) and all(s.sum_w >= 1.0 and s.nonfinite == 0 for s in st)
    check_batch_shift("%s underflow" % (kernel or "default"), bat, plist, ["graded"] * B, noms, seeds, 0, u, st)
    bat.close()


# 3. bit-exact properties with shift on ---------------------------------------------------------------------------------
def bits(bat, b, u, st):
    return (u[b].tobytes(), BS.stats_tuple(st[b]), bat.read_costs(b).tobytes(), bat.read_weights(b).tobytes())


def test_instance_of_a_batch_equals_the_batch_of_one():
    p = configs.diff_drive_defaults(1000, 15)
    B = 6
    assert family_code(None, p.model, 1000, B) == family_code(None, p.model, 1000, 1) == capi.BATCH_KERNEL_FOUR_WAVE
    seq = BS.varied(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    bat = BatchController(seq, B, min_shift=True)
    bat.set_nominal(nom)
    ones = [BatchController([seq[b]], 1, min_shift=True) for b in range(B)]
    for b, g in enumerate(ones):
        g.set_nominal(nom[b:b + 1])
    for it in range(2):
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        for b, g in enumerate(ones):
            u1, s1 = g.iterate(x0[b:b + 1], dt[b:b + 1], xr[b:b + 1], yr[b:b + 1], yaw0[b:b + 1], seeds[b:b + 1], it)
            assert bits(bat, b, u, st) == bits(g, 0, u1, s1)
    assert bat.last_kernel() == SV | capi.BATCH_KERNEL_FOUR_WAVE
    BS.close_all(bat, ones)


def test_one_instances_inputs_change_no_bit_of_another():
    p = configs.diff_drive_defaults(1000, 15)
    B, j = 6, 2
    seq = BS.varied(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    x2, xr2, yr2, seeds2, seq2 = x0.copy(), xr.copy(), yr.copy(), seeds.copy(), list(seq)
    x2[j] += (0.3, -0.2, 0.05)
    xr2[j] += 0.1
    yr2[j] -= 0.1
    seeds2[j] ^= np.uint64(0x5555)
    seq2[j] = seq[j].with_(control_noise=0.9, lam=0.05, v_ref=0.3, u_min=(-0.4, -1.1), u_max=(0.9, 1.3), path_weight=3.0)
    a, b = BatchController(seq, B, min_shift=True), BatchController(seq2, B, min_shift=True)
    for h in (a, b):
        h.set_nominal(nom)
    for it in range(2):
        ua, sa = a.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        ub, sb = b.iterate(x2, dt, xr2, yr2, yaw0, seeds2, it)
    assert not np.array_equal(ua[j], ub[j])
    for i in range(B):
        if i != j:
            assert bits(a, i, ua, sa) == bits(b, i, ub, sb)
    BS.close_all(a, b)


def test_copies_of_the_configuration_null_and_switching_off():
    """A handle without _set_params equals the handle given B copies of its configuration; _set_params(NULL) keeps the shift;
    switching the mode off reproduces the shift-off bits of a fresh handle."""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    plain, copies, fresh = (BatchController(p, B, min_shift=True), BatchController([p] * B, B, min_shift=True),
                            BatchController(p, B))
    for h in (plain, copies, fresh):
        h.set_nominal(nom)
    for it in range(2):
        ua, sa = plain.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        ub, sb = copies.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        for b in range(B):
            assert bits(plain, b, ua, sa) == bits(copies, b, ub, sb)
    assert plain.last_kernel() == copies.last_kernel() == SV | capi.BATCH_KERNEL_FOUR_WAVE
    copies.set_params(None)
    assert copies.get_min_shift()
    ua, sa = plain.iterate(x0, dt, xr, yr, yaw0, seeds, 2)
    ub, sb = copies.iterate(x0, dt, xr, yr, yaw0, seeds, 2)
    assert copies.last_kernel() == SV | capi.BATCH_KERNEL_FOUR_WAVE
    for b in range(B):
        assert bits(plain, b, ua, sa) == bits(copies, b, ub, sb)
    # off again: a fresh handle's kernels and bits from the same warm start
    plain.set_min_shift(False)
    assert not plain.get_min_shift()
    plain.set_nominal(nom)
    for it in range(2):
        ua, sa = plain.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        uf, sf = fresh.iterate(x0, dt, xr, yr, yaw0, seeds, it)
        for b in range(B):
            assert bits(plain, b, ua, sa) == bits(fresh, b, uf, sf)
    assert plain.last_kernel() == fresh.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    BS.close_all(plain, copies, fresh)


# 4. the resident loop -------------------------------------------------------------------------------------------------
def test_resident_loop_with_shift_equals_the_host_prologue():
    """55 advancing ticks (56 in all): index, window, pose, trace and u* of the resident batch equal the host prologue
    (calc_ref_path, plant_step) driving ccv_mppi_batch_iterate on a batch in the same mode, bit for bit."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 6, 56
    seq = BS.varied(p, B)
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    host = BatchController(seq, B, min_shift=True)
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
    bat = BatchController(seq, B, min_shift=True)
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
    assert bat.last_kernel() == SV | capi.BATCH_KERNEL_FOUR_WAVE
    for b in range(B):
        tr = bat.resident_read_trace(b)
        np.testing.assert_array_equal(tr[:, :p.nstate], np.array([r[0][b] for r in ref]))
        np.testing.assert_array_equal(tr[:, 5], np.array([r[1][b] for r in ref], dtype=float))
    bat.close()


@pytest.mark.parametrize("varied", [False, True], ids=["shared", "varied"])
@pytest.mark.parametrize("model,K,H,B", [("diff_drive", 1000, 15, 3), ("steering_diff_drive", 1000, 17, 8), ("diff_drive", 65537, 15, 2)])
def test_shift_resident_tick_pair(model, K, H, B, varied):
    """test_gpu_update.test_batch_resident_tick_pair in shifted-weight mode: tick 0's update runs inside
    k_finalize_advance_batch_shift, whose extra block forms the command that moves the pose, and tick 1 samples around the u*
    its finalize waves wrote; Y's tick-1 read-backs must fit the samples rebuilt around X's flushed u0 under check 1."""
    p = MODEL_DEFAULTS[model](K, H)
    paths = [amd.make_path("sinusoid" if b % 2 == 0 else "dkan") for b in range(B)]
    s0 = np.zeros((B, p.nstate))
    for b in range(B):
        i = 7 * b + 3
        s0[b, 0], s0[b, 1] = paths[b][0][i], paths[b][1][i] + 0.05
        s0[b, 2] = np.arctan2(paths[b][1][i + 1] - paths[b][1][i], paths[b][0][i + 1] - paths[b][0][i])
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)

    def make(params, shift=True):
        bat = BatchController(params, B, min_shift=shift)
        bat.resident_set_paths(paths)
        bat.resident_set_poses(s0, seeds)
        return bat

    probe = make(p, shift=False)
    probe.resident_step_enqueue(p.dt, 0, advance=False)
    probe.synchronize()
    lk = UC.lambdas_for([probe.read_costs(b) for b in range(B)], varied)
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
    check_batch_shift(what + " tick0 (flush)", X, plist, kinds, np.zeros((B, H - 1, p.udim)), seeds, 0, u0)
    Y.resident_step_enqueue(p.dt, 0, advance=False)
    Y.resident_step_enqueue(p.dt, 1, advance=True)
    u1 = Y.get_nominal()
    check_batch_shift(what + " tick1 (after the fused finalize)", Y, plist, kinds, u0, seeds, 1, u1)
    assert Y.last_kernel() & SV == SV
    # the pose Y moved to is the plant's step with the command X's finalize stored
    want = np.array([amd.plant_step(p.model, s0[b], u0[b][0], p.dt) for b in range(B)])
    np.testing.assert_array_equal(Y.resident_read()[0], want)
    BS.close_all(X, Y)


def test_resident_batch_stays_finite_where_lambda_underflows():
    """Odd instances get lambda = (their first tick's min cost) / 900, beyond the plain weights' underflow; with shift on every
    pose and every trace row of a 40-tick resident run is finite, and u* too."""
    p = configs.diff_drive_defaults(1000, 15)
    B, ticks = 6, 40
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    probe = BatchController(p, B)
    probe.resident_set_paths(paths)
    probe.resident_set_poses(s0, seeds)
    probe.resident_step_enqueue(p.dt, 0, advance=False)
    c0 = [probe.read_costs(b) for b in range(B)]
    probe.close()
    seq = [p.with_(lam=float(c0[b].min()) / 900.0) if b % 2 else p for b in range(B)]
    for b in range(1, B, 2):
        assert np.all(np.exp(-c0[b] / seq[b].lam) == 0.0)
    bat = BatchController(seq, B, min_shift=True)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    for it in range(ticks):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
    st = bat.resident_read()[0]
    assert np.all(np.isfinite(st)) and np.all(np.isfinite(bat.get_nominal()))
    for b in range(B):
        tr = bat.resident_read_trace(b)
        assert tr.shape[0] == ticks and np.all(np.isfinite(tr))
        assert np.hypot(*(tr[-1, :2] - tr[0, :2])) > 0.5    # (it drove)
    bat.close()


# 5. flush points, mixing, refusals, memory ---------------------------------------------------------------------------
def test_mode_switches_flush_a_pending_resident_update_and_mix_with_host_iterations():
    """resident steps, shift on, resident steps, a host-record iteration, _set_params(NULL), resident steps, shift off,
    resident steps: the same reads as the same sequence with a synchronisation after every step"""
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    seq = BS.varied(p, B)
    s0, seeds = BS.start_poses(p, B)
    x0, dt, xr, yr, yaw0, hseeds, _ = BS.instance_inputs(p, B)

    def run(sync):
        bat = BatchController(seq, B)
        bat.resident_set_paths([BS.path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, seeds)
        reads, kernels, it = [], [], 0

        def steps(n):
            nonlocal it
            for _ in range(n):
                bat.resident_step_enqueue(p.dt, it, advance=it > 0)
                it += 1
                if sync:
                    bat.synchronize()
            kernels.append(bat.last_kernel())

        steps(3)
        bat.set_min_shift(True)
        steps(3)
        reads.append(bat.get_nominal())
        reads.append(bat.resident_read()[0])
        steps(2)
        reads.append(bat.iterate(x0, dt, xr, yr, yaw0, hseeds, 100, want_stats=False))   # (sees the resident ticks' u*)
        steps(2)
        bat.set_params(None)
        steps(2)
        reads.append(bat.read_weights(B - 1))
        bat.set_min_shift(False)
        steps(2)
        reads.append(bat.read_costs(B - 1))
        reads.append(bat.get_nominal())
        reads.append(bat.resident_read()[0])
        bat.close()
        return reads, kernels

    (fused, kf), (plain, kp) = run(False), run(True)
    for a, b in zip(fused, plain):
        np.testing.assert_array_equal(a, b)
    r4, V = capi.BATCH_KERNEL_FOUR_WAVE, capi.BATCH_KERNEL_VARIED
    assert kf == kp == [r4 | V, r4 | SV, r4 | SV, r4 | SV, r4 | SV, r4]


def test_plain_family_is_refused_by_a_resident_step(monkeypatch):
    UC.set_kernel(monkeypatch, "v1")
    p = configs.diff_drive_defaults(256, 15)
    B = 3
    s0, seeds = BS.start_poses(p, B)
    bat = BatchController(p, B, min_shift=True)
    bat.resident_set_paths([BS.path_of(b) for b in range(B)])
    bat.resident_set_poses(s0, seeds)
    with pytest.raises(MPPIError) as e:
        bat.resident_step_enqueue(p.dt, 0, advance=False)
    assert e.value.code == capi.ERR_STATE
    st = bat.resident_read()
    np.testing.assert_array_equal(st[0], s0)
    assert st[5] == 0 and bat.get_min_shift()
    bat.close()


@pytest.mark.parametrize("kernel", [None, "v1"])
def test_shift_mode_returns_all_device_memory(monkeypatch, kernel):
    import torch
    UC.set_kernel(monkeypatch, kernel)
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    inputs = BS.instance_inputs(p, B)

    def cycle():
        bat = BatchController(p, B, min_shift=True)
        bat.iterate(*inputs[:6], 0)
        bat.read_weights(B - 1)
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
    bat = BatchController(p, B, min_shift=True)
    bat.iterate(*inputs[:6], 0)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for i in range(300):
        bat.set_min_shift(i % 2 == 1)
        if i % 7 == 0:
            bat.iterate(*inputs[:6], i)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 2 * 2**20
    bat.close()

"""GPU tests (-m gpu): the window pruning of the rollout kernels (pc_prune_window) held exact at its bisectors, boxes and hull
edges (the specification: tests/prune_reference.py, the probe windows and the permutation argument:
tests/prune_probe.py, whose docstrings have the idea; tests/test_prune_reference.py shows every wrong version caught on the CPU).

The method is tests/edge_probe.py's: iteration 0 from a fixed warm start with a harmless window, the stored states read back --
they do not depend on the window, asserted on every later run --, the probe windows built from the states of one wave's block,
the same iteration again.  The pose is the origin, so the stored absolute states ARE the relative positions the pruning works
with (the kernels keep positions relative to the pose in LDS; the staged ones, absolute, subtract the pose first: x - 0.0 is x).
Everything but the path term is silent, w_path = 1: a sample's cost is the sum over its states of clamp(d^2).

  single handles   CCV_MPPI_PRUNE=1 against =0, same kernel: costs, weights, sum_w and u* equal in every bit on every probe; and
                   the live sample's cost differs in bits from a =0 run of the window with the live point replaced by a copy of
                   the dominator: the probe reached the device.
  batch handles    no switch there: the probe window against its permutation with two survivors at 0 and H - 1, for which the
                   model's hull is [0, H4) in every block of every wave (asserted) -- the full loop.  B = 2, instance 1 carries
                   the probe; every rung of tests/test_gpu_batch_forms.py, the disc and grid terms with their weights on;
                   last_kernel() asserted at each.  On the plain rung also equal to the single handle's =0 costs.
  zero noise       control_noise = 0: all lanes coincide, every state's box is a point; the single survivor, the pose point and
                   window points on the block's own states for every block, the one-state tail block included; single handles
                   through the switch, a batch handle against its permutations.
  the switch       a window that keeps more than 3/4 in block 0 (the wave stops testing) and one that is prunable in block 0 and
                   keeps everything in block 1; the model's trace is printed.
  longdouble       the costs of every single-handle probe against sum_k clamp(min_j |p_k - r_j|^2) over the read-back states in
                   np.longdouble -- a yardstick that does not use the kernel's own full loop.  The bound, per sample, u = 2^-53:
                     f_j(p)   c_j = fl(fl(x^2) + fl(y^2)): 2 u c_j;  a_j, b_j exact;  the inner fma u |b py + c|, the outer u |f|:
                              together below 4 u S_j, S_j = |a_j px| + |b_j py| + c_j
                     minimum  the computed minimum lies between the true one minus and plus the largest such error among the
                              points within 1e-9 (relative) of the nearest: e_k = 4 u max S_j over those
                     |p|^2    fma(px, px, fl(py^2)): u py^2 + u |p|^2 <= 2 u |p|^2
                     d^2      fl(m + |p|^2): u d^2;  the clamp is exact;  w = 1: the product is exact inside the fma
                     the sum  over N states in any partition: (N - 1) u sum_k d^2_k
                   bound = 1.01 (sum_k (e_k + 2 u |p_k|^2 + u d^2_k) + (N - 1) u sum_k d^2_k) -- derived, not tuned; error over
                   bound is printed per case.  A ladder rung whose eps is below the bound of its sample cannot be seen by this
                   check; their share is printed, and none of them may be a rung above 2^8.

-s prints the counts."""
import numpy as np
import pytest

import batch_support as BS
import prune_probe as PP
import prune_reference as PR
from ccv_mppi_path_tracker_amd import BatchController, MPPIController, capi

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
SEED = 11
VARIED, SHIFT = capi.BATCH_KERNEL_VARIED, capi.BATCH_KERNEL_SHIFT
OBST, MOVING, GRID = capi.BATCH_KERNEL_OBST, capi.BATCH_KERNEL_MOVING, capi.BATCH_KERNEL_GRID


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def path_only(model, K, H):
    p = BS.MODEL_DEFAULTS[model](K, H)
    return p.with_(path_weight=1.0, v_weight=0.0, zmp_weight=0.0, roll_v_weight=0.0, back_weight=0.0, yaw_weight=0.0)


def warm_start(p):
    """forward at three quarters of the speed range, everything else mid-range: the samples fan out ahead of the pose"""
    lo, hi = np.array(p.u_min), np.array(p.u_max)
    nom = np.tile((hi + lo) / 2, (p.horizon - 1, 1))
    nom[:, 0] += 0.25 * (hi[0] - lo[0])
    return nom


def nstates(p):
    return p.horizon - 2 if p.model == "full_body" else p.horizon


def pose(p, xy=(0.0, 0.0)):
    s = np.zeros(p.nstate)
    s[:3] = xy[0], xy[1], 0.3
    return s


def harmless(p, xy=(0.0, 0.0)):
    k = np.arange(p.horizon)
    return xy[0] + 0.06 * k * np.cos(0.3), xy[1] + 0.06 * k * np.sin(0.3)


def run_single(g, p, x0, nom, win):
    g.set_nominal(nom)
    u, st = g.iterate(x0, p.dt, win[0], win[1], 0.3, SEED, 0)
    return dict(u=u.copy(), sum_w=st.sum_w, c=g.read_costs(), w=g.read_weights(), xy=g.read_candidates())


def same(a, b):
    return (all(a[k].tobytes() == b[k].tobytes() for k in ("u", "c", "w", "xy"))
            and np.float64(a["sum_w"]).tobytes() == np.float64(b["sum_w"]).tobytes())


def wave_states(xy, wave, T):
    P = xy[64 * wave:64 * wave + 64, :T]
    assert P.shape[0] == 64 and np.all(np.isfinite(P)), "the wave's states are not 64 finite rollouts"
    return P


def edges_alone(px, py):
    """one position alone attains each edge of the block, with room for the widest rung's bisector"""
    return all((PP.extreme(px, py, s) or (0, 0.0))[1] > 1.0e-6 for s in PP.SIDES)


def gap_probes(px, py, H):
    """the fp32-gap probes the block carries: one per edge that rounds inwards and for which the builder's promises can be had"""
    out = []
    for s in PP.SIDES:
        if PP.fp32_rounds_inwards(px, py, s):
            try:
                out.append(PP.fp32_gap(px, py, H, s))
            except AssertionError:
                pass
    return out


def choose_block(xy, waves, T, H):
    """(wave, block, its fp32-gap probes): of the given waves' blocks after block 0 (whose state 0 every lane shares), the first
    in which one position alone attains each edge and which carries an fp32-gap probe -- the one probe the outward step of
    the box alone holds"""
    for wave in waves:
        P = wave_states(xy, wave, T)
        for bn in range(1, (T + 7) // 8):
            px, py = PP.block_of(P, bn, T)
            if edges_alone(px, py):
                gaps = gap_probes(px, py, H)
                if gaps:
                    return wave, bn, gaps
    raise AssertionError("no block with every edge attained alone that carries an fp32-gap probe")


def probe_list(px, py, H, full, gaps):
    """the probes of one case: the whole ladder on xhi, three rungs on the other edges, the block's fp32 gaps, the hull edges
    (`full`; else four of them), the two live points, the single survivor"""
    out = [PP.ladder(px, py, H, "xhi", k) for k in PP.RUNGS]
    out += [PP.ladder(px, py, H, s, k) for s in PP.SIDES[1:] for k in (2, 10, 30)]
    out += gaps
    cases = PP.edge_cases(H)
    out += [PP.edge(px, py, H, *c) for c in (cases if full else cases[::max(1, len(cases) // 4)])]
    out.append(PP.two_live(px, py, H)[0])
    out.append(PP.single_survivor(px, py, H))
    return out


def longdouble_cost(P, xr, yr):
    """(cost [K], bound [K]) over the states P [K][T][2] (module docstring)"""
    x, y = P[..., 0].astype(LD)[..., None], P[..., 1].astype(LD)[..., None]
    d2 = (x - xr.astype(LD)) ** 2 + (y - yr.astype(LD)) ** 2                      # [K][T][H]
    dmin = d2.min(axis=2)
    near = d2 <= dmin[..., None] * (1 + LD(1e-9)) + LD(1e-300)
    S = np.abs(2 * xr * P[..., 0:1]) + np.abs(2 * yr * P[..., 1:2]) + (xr * xr + yr * yr)
    e = 4 * U * np.where(near, S, 0.0).max(axis=2)
    pp = P[..., 0] ** 2 + P[..., 1] ** 2
    dc = np.minimum(np.maximum(dmin, 0), LD(1.0e4))
    T = P.shape[1]
    bound = 1.01 * ((e + 2 * U * pp + U * dc.astype(np.float64)).sum(axis=1) + (T - 1) * U * dc.astype(np.float64).sum(axis=1))
    return dc.sum(axis=1), bound


# ---- single handles ------------------------------------------------------------------------------------------------------
SINGLE = [("diff_drive", None, 128, 17, True), ("diff_drive", None, 100, 20, False), ("diff_drive", None, 128, 50, False),
          ("diff_drive", "r3", 128, 65, True), ("diff_drive", "pc", 128, 68, False), ("diff_drive", "solo", 128, 128, True),
          ("steering_diff_drive", None, 128, 20, False), ("steering_diff_drive", "r3", 128, 50, False),
          ("steering_diff_drive", "pc", 128, 68, False), ("steering_diff_drive", "solo", 128, 17, False), ("full_body", None, 128, 20, False), ("full_body", "pc", 128, 65, False),
          ("full_body", "solo", 128, 50, False)]


@pytest.mark.parametrize("model,kernel,K,H,full", SINGLE, ids=["%s-%s-K%d-H%d" % (c[0], c[1] or "default", c[2], c[3]) for c in SINGLE])
def test_pruned_loop_equals_full_loop_on_every_probe(monkeypatch, model, kernel, K, H, full):
    p = path_only(model, K, H)
    T, x0, nom = nstates(p), pose(p), warm_start(p)
    if kernel:
        monkeypatch.setenv("CCV_MPPI_KERNEL", kernel)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "1")
    on = MPPIController(p)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "0")
    off = MPPIController(p)
    base = run_single(on, p, x0, nom, harmless(p))
    assert run_single(on, p, x0, nom, harmless(p))["xy"].tobytes() == base["xy"].tobytes(), "the states of two runs differ"
    assert same(base, run_single(off, p, x0, nom, harmless(p)))
    # (K = 100: wave 1 is the masked one -- the positions of its idle lanes are not stored, so no window can be built for its
    #  box; it is compared on the windows built for wave 0)
    wave, bn, gaps = choose_block(base["xy"], (1, 0) if K >= 128 else (0,), T, H)
    P = wave_states(base["xy"], wave, T)
    px, py = PP.block_of(P, bn, T)
    probes = probe_list(px, py, H, full, gaps)
    worst, blind, small, reached = 0.0, [], 0, 0
    for pr in probes:
        a, b = run_single(on, p, x0, nom, (pr.xr, pr.yr)), run_single(off, p, x0, nom, (pr.xr, pr.yr))
        assert a["xy"].tobytes() == base["xy"].tobytes(), pr.what
        assert same(a, b), (pr.what, np.flatnonzero(a["c"] != b["c"])[:8])
        co = PR.window_coeffs(pr.xr, pr.yr)
        jb, je, _, _ = PR.device_hull(px, py, co[0], co[1], co[2], H)
        small += int(je - jb < PR.h4_of(H))
        if np.isfinite(pr.margin):   # the probe is live on the device: without the live point the sample's cost has other bits
            xr2, yr2 = pr.xr.copy(), pr.yr.copy()
            dead = [pr.j] + ([H - 2] if pr.what.startswith("two live") else [])
            xr2[dead], yr2[dead] = pr.xr[pr.r], pr.yr[pr.r]
            c2 = run_single(off, p, x0, nom, (xr2, yr2))["c"]
            i = 64 * wave + pr.star % 64
            if pr.margin > 4.0 * np.spacing(b["c"][i]):   # (a margin below the last place of the sample's whole cost may vanish in its sum)
                assert c2[i].tobytes() != b["c"][i].tobytes(), (pr.what, "the probe did not reach the device", float(c2[i]))
                reached += 1
        ref, bound = longdouble_cost(P, pr.xr, pr.yr)   # (the probe's wave)
        err = np.abs((a["c"][64 * wave:64 * wave + 64].astype(LD) - ref).astype(np.float64))
        assert np.all(err <= bound), (pr.what, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
        if pr.what.startswith("ladder") and pr.eps < bound[pr.star % 64]:
            blind.append(pr.what)
    print("[prune] %s %s K=%d H=%d: wave %d block %d, %d probes bit-equal (%d with a hull below H4), error over bound %.3f, "
          "rungs below the longdouble bound: %d of %d %s" % (model, kernel or "default", K, H, wave, bn, len(probes), small, worst,
                                                            len(blind), sum(q.what.startswith("ladder") for q in probes), blind))
    print("[prune] ... %d probes shown live on the device, %d of them fp32-gap probes" % (reached, len(gaps)))
    assert small >= len(probes) - 1, "the probes do not prune"
    # (the rungs 2^24 .. 2^30 of the xhi ladder are above four ulps of any cost below 2^20 |p*|^2: at least those four)
    assert reached >= 4, "too few probes reach the device: %d" % reached
    if H <= 20:   # (the bound grows with N sum d^2: the ladder is this check's at the short horizons; beyond them the share is printed)
        assert all(int(w.split("k=")[1].split()[0]) <= 8 for w in blind), blind
    on.close()
    off.close()


def test_pose_point_and_off_origin(monkeypatch):
    """the pose itself as a window point, three times (T = 0 against itself; a minimum that is a zero: compared through the
    switch only), and one case off the origin, device against device: there the stored states are not the relative positions,
    the probe is built from their difference to the pose and only the equality of the two loops is asserted"""
    model, K, H = "diff_drive", 128, 20
    p = path_only(model, K, H)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "1")
    on = MPPIController(p)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "0")
    off = MPPIController(p)
    nom = warm_start(p)
    for xy in ((0.0, 0.0), (3.7, -1.3)):
        x0 = pose(p, xy)
        base = run_single(on, p, x0, nom, harmless(p, xy))
        P = wave_states(base["xy"], 1, H) - np.array(xy)
        for bn in (0, 1):
            px, py = PP.block_of(P, bn, H)
            wins = [PP.pose_point(px, py, H)]
            if bn == 1:
                wins += [PP.ladder(px, py, H, "xhi", k, check=xy == (0.0, 0.0)) for k in (2, 10, 30)]
            for pr in wins:
                win = (pr.xr + xy[0], pr.yr + xy[1])
                a, b = run_single(on, p, x0, nom, win), run_single(off, p, x0, nom, win)
                assert same(a, b), (xy, bn, pr.what)
    on.close()
    off.close()


ZERO_NOISE = [("diff_drive", None, 128, 17), ("diff_drive", "solo", 128, 65), ("full_body", None, 128, 20)]


def coincident_windows(px, py, H):
    return [PP.single_survivor(px, py, H), PP.single_survivor(px, py, H, twin=True), PP.pose_point(px, py, H), PP.on_states(px, py, H)]


@pytest.mark.parametrize("model,kernel,K,H", ZERO_NOISE, ids=["%s-%s-H%d" % (c[0], c[1] or "default", c[3]) for c in ZERO_NOISE])
def test_zero_noise_launch_where_all_lanes_coincide(monkeypatch, model, kernel, K, H):
    """control_noise = 0: every sample is the warm start's rollout, every state's box is one point (asserted on the stored
    states), and the tail block of H = 17 and 65 is a single point altogether: only the one-sided outward step lies between
    the box and the positions.  The single survivor, its twin, the pose point and window points ON the block's first and last
    state, built for every block in turn, CCV_MPPI_PRUNE=1 against =0"""
    p = path_only(model, K, H).with_(control_noise=0.0)
    T, x0, nom = nstates(p), pose(p), warm_start(p)
    if kernel:
        monkeypatch.setenv("CCV_MPPI_KERNEL", kernel)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "1")
    on = MPPIController(p)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "0")
    off = MPPIController(p)
    base = run_single(on, p, x0, nom, harmless(p))
    xy = base["xy"][:, :T]
    assert np.all(np.isfinite(xy)) and all(xy[i].tobytes() == xy[0].tobytes() for i in range(K)), "the samples do not coincide"
    assert len({xy[0, k].tobytes() for k in range(T)}) == T, "the rollout does not move"
    n = 0
    for bn, (px, py) in enumerate(PP.blocks_of(wave_states(base["xy"], 1, T), T)):
        for pr in coincident_windows(px, py, H):
            a, b = run_single(on, p, x0, nom, (pr.xr, pr.yr)), run_single(off, p, x0, nom, (pr.xr, pr.yr))
            assert a["xy"].tobytes() == base["xy"].tobytes(), (bn, pr.what)
            assert same(a, b), (bn, pr.what, float(a["c"][0]), float(b["c"][0]))
            n += 1
    print("[prune] zero noise %s %s H=%d: %d windows over %d blocks bit-equal, tail block of %d state(s)"
          % (model, kernel or "default", H, n, (T + 7) // 8, T - 8 * ((T - 1) // 8)))
    on.close()
    off.close()


def test_zero_noise_batch_equals_its_permutation():
    """the same launch on a batch handle (B = 2, H = 17: the tail block is one point): the twin survivor and the points on the
    block's states against their full-hull permutations"""
    model, K, H, B = "diff_drive", 128, 17, 2
    p = path_only(model, K, H).with_(control_noise=0.0)
    bat = BatchController(p, B)
    base = run_batch(bat, batch_inputs(p, B, harmless(p)))
    xy = base[1]["xy"]
    assert all(xy[i].tobytes() == xy[0].tobytes() for i in range(K)), "the samples do not coincide"
    waves = [PP.blocks_of(wave_states(xy, w, H), H) for w in (0, 1)]
    n = 0
    for bn, (px, py) in enumerate(waves[1]):
        # (block 0's first state is the pose: a window point on it makes the minimum a zero, whose sign depends on the order)
        for pr in [PP.single_survivor(px, py, H, twin=True)] + ([PP.on_states(px, py, H)] if bn else []):
            xp, yp, _ = PP.permuted(pr.xr, pr.yr, [w[0] for w in waves], H)
            co = PR.window_coeffs(xp, yp)
            for w in waves:
                trace = PR.switch_trace(w, co[0], co[1], co[2], H)
                assert all(t[:2] == (0, PR.h4_of(H)) for t in trace), (bn, pr.what, trace)
            a, b = run_batch(bat, batch_inputs(p, B, (pr.xr, pr.yr))), run_batch(bat, batch_inputs(p, B, (xp, yp)))
            assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE, hex(bat.last_kernel())
            for i in (0, 1):
                assert a[i]["xy"].tobytes() == base[i]["xy"].tobytes() and a[i]["c"].tobytes() == b[i]["c"].tobytes(), (bn, pr.what, i)
            n += 1
    print("[prune] zero noise batch: %d windows equal their full-hull permutations" % n)
    bat.close()


# ---- the switch ------------------------------------------------------------------------------------------------------------
def test_the_switch_ends_the_testing(monkeypatch):
    model, K, H = "diff_drive", 128, 50
    p = path_only(model, K, H)
    x0, nom = pose(p), warm_start(p)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "1")
    on = MPPIController(p)
    monkeypatch.setenv("CCV_MPPI_PRUNE", "0")
    off = MPPIController(p)
    base = run_single(on, p, x0, nom, harmless(p))
    waves = [PP.blocks_of(wave_states(base["xy"], w, H)) for w in (0, 1)]
    H4 = PR.h4_of(H)
    # 1. two survivors of block 0 at 0 and H - 1: block 0 keeps everything, the wave stops testing; the points are a ladder's on
    #    block 3, prunable there
    px, py = waves[1][3]
    lad = PP.ladder(px, py, H, "xhi", 10)
    xr, yr, _ = PP.permuted(lad.xr, lad.yr, [w[0] for w in waves], H)
    # 2. the dominator and its twin at 0 and 1, the live point of block 1 at H - 1: block 0 keeps four points, block 1 everything
    px, py = waves[1][1]
    lad1 = PP.ladder(px, py, H, "xhi", 10, j=H - 1, r=0, twin=1)
    for name, win, want in (("full at block 0", (xr, yr), 0), ("full at block 1", (lad1.xr, lad1.yr), 1)):
        co = PR.window_coeffs(*win)
        trace = PR.switch_trace(waves[1], co[0], co[1], co[2], H)
        print("[prune] switch, %s: wave 1 (jb, je, tested) %s" % (name, trace))
        assert trace[want][:2] == (0, H4) and trace[want][2] and not any(t[2] for t in trace[want + 1:]), (name, trace)
        assert all(t[1] - t[0] < H4 for t in trace[:want]), (name, trace)
        a, b = run_single(on, p, x0, nom, win), run_single(off, p, x0, nom, win)
        assert a["xy"].tobytes() == base["xy"].tobytes() and same(a, b), name
    on.close()
    off.close()


# ---- batch handles -----------------------------------------------------------------------------------------------------------
def run_batch(bat, inputs):
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat.set_nominal(nom)
    bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    return [dict(c=bat.read_costs(b), w=bat.read_weights(b), xy=bat.read_candidates(b)) for b in (0, 1)]


def batch_inputs(p, B, win1):
    xr, yr = np.tile(harmless(p)[0], (B, 1)), np.tile(harmless(p)[1], (B, 1))
    xr[1], yr[1] = win1
    x0 = np.tile(pose(p), (B, 1))
    seeds = np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64)
    return x0, np.full(B, p.dt), xr, yr, np.full(B, 0.3), seeds, np.tile(warm_start(p), (B, 1, 1))


def probe_and_twin(bat, p, B, waves_of):
    """the states of instance 1 under the handle's present settings -> [(what, probe window, permuted window)], the model's
    hulls asserted: below H4 in the probe's block, [0, H4) in every block of every wave for the permuted order"""
    H, T = p.horizon, nstates(p)
    base = run_batch(bat, batch_inputs(p, B, harmless(p)))
    waves = [PP.blocks_of(wave_states(base[1]["xy"], w, T), T) for w in range(waves_of)]
    wave, bn, gaps = choose_block(base[1]["xy"], range(waves_of - 1, -1, -1), T, H)
    px, py = waves[wave][bn]
    out = []
    for pr in [PP.ladder(px, py, H, "xhi", k) for k in (2, 6, 10, 20, 30)] + [PP.ladder(px, py, H, "ylo", 10), PP.two_live(px, py, H)[0]] \
            + gaps[:1] \
            + [PP.edge(px, py, H, *c) for c in PP.edge_cases(H)[::5]]:
        co = PR.window_coeffs(pr.xr, pr.yr)
        jb, je, _, _ = PR.device_hull(px, py, co[0], co[1], co[2], H)
        assert je - jb < PR.h4_of(H) or pr.what.startswith("two live"), (pr.what, jb, je)   # (those span the window)
        xp, yp, _ = PP.permuted(pr.xr, pr.yr, [w[0] for w in waves], H)
        co = PR.window_coeffs(xp, yp)
        for w in waves:
            trace = PR.switch_trace(w, co[0], co[1], co[2], H)
            assert all(t[:2] == (0, PR.h4_of(H)) for t in trace), (pr.what, trace)
        out.append((pr.what, (pr.xr, pr.yr), (xp, yp)))
    return base, out


@pytest.mark.parametrize("model,K,H", [("diff_drive", 128, 17), ("diff_drive", 128, 20), ("full_body", 64, 20)])
def test_batch_probe_equals_its_full_hull_permutation_on_every_rung(monkeypatch, model, K, H):
    B = 2
    p = path_only(model, K, H)
    assert BS.families(model, K, B)[1] == "r4"
    bat = BatchController(p, B)
    x0 = pose(p)
    discs = [np.array([[0.3, 0.1, 0.3]]), np.array([[0.2, 0.0, 0.25], [0.5, 0.1, 0.2]])]
    velocities = [np.array([[0.1, -0.05]]), np.array([[-0.08, 0.06], [0.0, 0.1]])]
    cells = (0.25 + np.random.default_rng(7).random((24, 24))).astype(np.float32)
    maps = [(cells, (-3.0, -3.0), 0.25, 0.5), (cells.T.copy(), (-3.0, -3.0), 0.25, 0.0)]
    lam = [p.with_(lam=p.lam * (0.5 + 0.3 * b)) for b in range(B)]   # (lambda alone: the states stay, the VARIED kernels run)
    rungs = [(0, lambda: None), (VARIED, lambda: bat.set_params(lam)), (SHIFT, lambda: bat.set_min_shift(True)),
             (OBST, lambda: bat.set_obstacles(discs, 5.0)), (MOVING, lambda: bat.set_obstacle_velocities(velocities)),
             (GRID, lambda: bat.set_grids(maps, [0, 1], [0.01, 0.025]))]
    bits, first = capi.BATCH_KERNEL_FOUR_WAVE, None
    for add, do in rungs:
        do()
        bits |= add
        base, pairs = probe_and_twin(bat, p, B, (K + 63) // 64)
        first = first or base
        assert base[1]["xy"].tobytes() == first[1]["xy"].tobytes(), hex(bits)
        for what, win, twin in pairs:
            a, b = run_batch(bat, batch_inputs(p, B, win)), run_batch(bat, batch_inputs(p, B, twin))
            assert bat.last_kernel() == bits, (what, hex(bat.last_kernel()), hex(bits))
            for i in (0, 1):
                assert a[i]["xy"].tobytes() == base[i]["xy"].tobytes(), (hex(bits), what, i)
                assert a[i]["c"].tobytes() == b[i]["c"].tobytes(), (hex(bits), what, i, np.flatnonzero(a[i]["c"] != b[i]["c"])[:8])
                assert a[i]["w"].tobytes() == b[i]["w"].tobytes(), (hex(bits), what, i)
            if add == 0:   # the plain rung: the single handle's full loop
                monkeypatch.setenv("CCV_MPPI_PRUNE", "0")
                g = MPPIController(p)
                g.set_nominal(warm_start(p))
                g.iterate(x0, p.dt, win[0], win[1], 0.3, BS.instance_seed(1), 0)
                assert g.read_costs().tobytes() == a[1]["c"].tobytes(), what
                g.close()
        print("[prune] batch %s K=%d H=%d kernel %#x: %d probes equal their full-hull permutations" % (model, K, H, bits, len(pairs)))
    bat.close()


def test_one_wave_batch_probe_equals_its_permutation():
    """the one-wave batch kernel, through the instance count the grid and moving suites use for it"""
    model, K, H = "diff_drive", 64, 17
    B = 5 * BS.cus() + 1
    p = path_only(model, K, H)
    assert BS.families(model, K, B)[1] == "solo"
    bat = BatchController(p, B)
    base, pairs = probe_and_twin(bat, p, B, 1)
    for what, win, twin in pairs:
        a, b = run_batch(bat, batch_inputs(p, B, win)), run_batch(bat, batch_inputs(p, B, twin))
        assert bat.last_kernel() == capi.BATCH_KERNEL_ONE_WAVE, hex(bat.last_kernel())
        for i in (0, 1):
            assert a[i]["xy"].tobytes() == base[i]["xy"].tobytes() and a[i]["c"].tobytes() == b[i]["c"].tobytes(), (what, i)
    print("[prune] one-wave batch, B = %d: %d probes equal their full-hull permutations" % (B, len(pairs)))
    bat.close()

"""GPU tests (-m gpu) of the single handle's feed: ccv_mppi_read_top_candidates (k_top_weights = top_weights() of
csrc/mppi_top_weights.h, the host ordering top_order_pairs(), k_gather_xy_list), ccv_mppi_read_candidates (k_gather_xy with a
stride) and ccv_mppi_read_weights (k_normalise_weights with first != 0).  DESIGN.md section 14.

Checkers: tests/top_reference.py (the order as numpy states it, and the kernel's own layout) for the selection behind
tests/probe/top_probe.hip on the inputs of tests/top_cases.py; through the C call, weights with CHOSEN ties -- samples dealt to
seven groups, every member of a group given the same injected controls -- where conditions asserted on the device's own
read-backs (costs bit-equal inside a group, weights strictly decreasing over the groups) make the expected list exact; the full
read-backs for the gathers.  Every comparison is of integers or of bit patterns: no tolerance, no timing.
"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import top_cases as Cs
import top_probe
import top_reference as R
from batch_support import MODEL_DEFAULTS
from ccv_mppi_path_tracker_amd import capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController, MPPIError

pytestmark = pytest.mark.gpu
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b, msg=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


# ---- 1. top_weights() and top_order_pairs() behind the probe, against the numpy reference ---------------------------------------
@pytest.mark.parametrize("K", Cs.KS)
def test_probe_gives_the_layout_the_order_and_the_bits(K):
    """Every input of top_cases at every count: three vectors per launch, the padding beyond K filled with NaN (which would come
    first if it were read).  The kernel's raw output is the reference's layout (greater than T in index order, then the
    lowest-index equal to T), the ordered result the reference's order, the weights their own bits, and a second launch writes the
    same bytes."""
    pitch = (K + 63) // 64 * 64 + 64   # (padding even where K is a multiple of 64)
    launches = 0
    for name, N, vecs in Cs.all_inputs(K):
        grid = np.full((3, pitch), np.nan)
        for s in range(3):
            grid[s, :K] = vecs[s]
        first = top_probe.top(grid, K, N)
        again = top_probe.top(grid, K, N)
        for s in range(3):
            what = "%s K=%d N=%d vector %d" % (name, K, N, s)
            lay_idx, lay_bits = R.kernel_layout(vecs[s], N)
            top_idx, top_bits = R.top(vecs[s], N)
            np.testing.assert_array_equal(first[0][s], lay_idx, err_msg="layout, " + what)
            np.testing.assert_array_equal(first[1][s], lay_bits, err_msg="layout bits, " + what)
            np.testing.assert_array_equal(first[2][s], top_idx, err_msg="order, " + what)
            np.testing.assert_array_equal(first[3][s], top_bits, err_msg="ordered bits, " + what)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), "second launch, %s K=%d N=%d" % (name, K, N)
        launches += 1
    print("K=%d: %d launches of three vectors, %d array comparisons" % (K, launches, launches * 16))


# ---- 2. through the C call: chosen ties -----------------------------------------------------------------------------------------
GROUPS = 7
TIE_K = (1000, 1025, 2049)
DEALS = ("both_sides", "random")
NAN_A, NAN_B = np.array([0x7FF8000000000000, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)


def tie_setup(K, deal):
    """(params, state, window, group [K], controls [K][H - 1][udim]): diff drive, H = 9; every sample of a group has the group's
    control sequence, drawn inside the bounds"""
    w = configs.workload("C2", num_samples=K, horizon=9)
    p = w.params
    path = helpers.oracle_path(w.path)
    state = np.zeros(p.nstate)
    state[0], state[1] = path[0][0], path[1][0] + 0.05
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    rng = np.random.default_rng(7000 + K + (0 if deal == "both_sides" else 1))
    lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
    seqs = lo + (hi - lo) * rng.uniform(0.05, 0.95, size=(GROUPS, p.horizon - 1, p.udim))
    group = np.arange(K) % GROUPS if deal == "both_sides" else rng.integers(0, GROUPS, size=K)
    for g in range(GROUPS):
        m = np.flatnonzero(group == g)
        assert m.size > 0
        if deal == "both_sides":   # members on both sides of 63|64 and of 1023|1024 (K = 1025 has one sample beyond: one group's)
            assert m[0] < 64 <= m[-1] and (K < 1024 + GROUPS or m[0] < 1024 <= m[-1])
    if deal == "both_sides" and K > 1024:
        assert np.any(group[:1024] == group[1024])
    return p, state, xr, yr, yaw[0], group, seqs[group]


def weighted(p, ctl, state, xr, yr, yaw0, lam, **kw):
    g = MPPIController(p.with_(lam=lam), **kw)
    g.inject_controls(ctl)
    g.predict_States(state, p.dt)
    g.calc_Weights(xr, yr, yaw0)
    return g


def group_costs(costs, group, members=None):
    """the groups' costs, asserted equal in every bit inside a group (over `members`, default all) and distinct between groups"""
    keep = np.ones(costs.size, dtype=bool) if members is None else members
    out = np.zeros(GROUPS)
    for g in range(GROUPS):
        c = costs[(group == g) & keep]
        assert c.size > 0 and np.all(bits(c) == bits(c[:1])[0]), "group %d: costs differ inside the group" % g
        out[g] = c[0]
    assert np.unique(out).size == GROUPS and np.all(np.isfinite(out))
    return out


def raw_top(g, count, with_paths=True, fill=-7.0):
    """ccv_mppi_read_top_candidates into buffers of K + 2 rows pre-filled with `fill`: (rc, idx, w, xy)"""
    idx = np.full(g.K + 2, -7, dtype=np.int32)
    w, xy = np.full(g.K + 2, fill), np.full((g.K + 2, g.H, 2), fill)
    rc = g.lib.ccv_mppi_read_top_candidates(g._h, int(count), idx.ctypes.data_as(i32p), capi.dptr(w), capi.dptr(xy) if with_paths else None)
    return rc, idx, w, xy


def check_top_calls(g, expected, what):
    """every count of the probe's list: idx, top_w non-increasing by key, every row of xy, with_paths=False, the rows beyond
    `count` untouched; count == 0 writes nothing; count == K + 1 is refused with the buffers untouched"""
    K = g.K
    full = g.read_candidates()
    for N in Cs.counts_for(K):
        rc, idx, w, xy = raw_top(g, N)
        assert rc == capi.OK, what
        np.testing.assert_array_equal(idx[:N], expected[:N], err_msg="%s N=%d" % (what, N))
        key = R.key(w[:N])
        assert np.all(key[1:] <= key[:-1]), "%s N=%d: top_w not in order" % (what, N)
        same_bits(xy[:N], full[idx[:N]], "%s N=%d rows" % (what, N))
        assert np.all(idx[N:] == -7) and np.all(w[N:] == -7.0) and np.all(xy[N:] == -7.0), "%s N=%d: wrote past count" % (what, N)
        rc, idx2, w2, xy2 = raw_top(g, N, with_paths=False)
        assert rc == capi.OK and np.all(xy2 == -7.0)
        np.testing.assert_array_equal(idx2, idx)
        same_bits(w2, w)
    for count, want in ((0, capi.OK), (K + 1, capi.ERR_INVALID_ARG)):
        rc, idx, w, xy = raw_top(g, count)
        assert rc == want, (what, count, rc)
        assert np.all(idx == -7) and np.all(w == -7.0) and np.all(xy == -7.0), "%s count=%d: buffers touched" % (what, count)
    return raw_top(g, K, with_paths=False)[2][:K]


@pytest.fixture(scope="module")
def tie_cases():
    made = {}

    def get(K, deal):
        if (K, deal) not in made:
            s = tie_setup(K, deal)
            g = weighted(s[0], s[6], *s[1:5], 1.0)
            made[(K, deal)] = s + (g.read_costs(),)
            g.close()
        return made[(K, deal)]
    return get


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("K", TIE_K)
def test_top_candidates_graded(tie_cases, K, deal):
    """lambda = (c_max - c_min) / ln 1000: seven distinct weights, each shared by a seventh of the samples"""
    p, state, xr, yr, yaw0, group, ctl, c0 = tie_cases(K, deal)
    lam = (c0.max() - c0.min()) / math.log(1000.0)
    g = weighted(p, ctl, state, xr, yr, yaw0, lam)
    costs = g.read_costs()
    gc = group_costs(costs, group)
    wn = g.read_weights()
    by_cost = np.argsort(gc)
    gw = np.array([wn[group == j][0] for j in by_cost])
    for j, v in zip(by_cost, gw):
        assert np.all(bits(wn[group == j]) == bits(v)), "group %d: weights differ inside the group" % j
    assert np.all(gw[1:] < gw[:-1]), "the groups' weights do not strictly decrease with their costs"
    expected = np.lexsort((np.arange(K), costs))
    top_w = check_top_calls(g, expected, "graded K=%d %s" % (K, deal))
    assert np.unique(bits(top_w)).size == GROUPS
    g.close()


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("K", TIE_K)
def test_top_candidates_flat(tie_cases, K, deal):
    """lambda = 1e300: every weight is exactly 1.0, one run of K equal keys; the answer is 0 .. N - 1"""
    p, state, xr, yr, yaw0, group, ctl, c0 = tie_cases(K, deal)
    g = weighted(p, ctl, state, xr, yr, yaw0, 1e300)
    group_costs(g.read_costs(), group)
    top_w = check_top_calls(g, np.arange(K), "flat K=%d %s" % (K, deal))
    assert np.all(top_w == 1.0)
    g.close()


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("K", TIE_K)
def test_top_candidates_underflow(tie_cases, K, deal):
    """MIN_SHIFT with lambda = (second-lowest group cost - c_min) / 800: the best group sits at exactly 1.0, every other weight is
    exp(-800 or less) = 0; beyond the best group the list goes on with the lowest-index zero-weight samples"""
    p, state, xr, yr, yaw0, group, ctl, c0 = tie_cases(K, deal)
    cs = np.unique(c0)
    lam = float(cs[1] - cs[0]) / 800.0
    assert lam > 0
    g = weighted(p, ctl, state, xr, yr, yaw0, lam, min_shift=True)
    _, st = g.determine_OptimalSolution(want_stats=True)
    costs = g.read_costs()
    gc = group_costs(costs, group)
    best = group == int(np.argmin(gc))
    assert st.n_zero_weight == K - int(best.sum())
    wn = g.read_weights()
    assert np.all(wn[~best] == 0.0) and np.all(wn[best] > 0.0)
    expected = np.concatenate([np.flatnonzero(best), np.flatnonzero(~best)])
    top_w = check_top_calls(g, expected, "underflow K=%d %s" % (K, deal))
    assert np.all(top_w[:best.sum()] == 1.0) and np.all(bits(top_w[best.sum():]) == 0)
    g.close()


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("K", TIE_K)
def test_top_candidates_with_nan_weights(tie_cases, K, deal):
    """Six samples get NaN controls, of two payloads (one of them negative): their costs and weights are NaN, and they come
    first, by sample index, whatever their patterns; behind them the graded order of the others.  sum_w is NaN here, so
    read_weights() says nothing; the others' weights are strictly ordered because exp() of the groups' costs, evaluated on the
    host, differs by more than 1e-6 relative between neighbours -- ten orders above any rounding of the device's exp."""
    p, state, xr, yr, yaw0, group, ctl, c0 = tie_cases(K, deal)
    lam = (c0.max() - c0.min()) / math.log(1000.0)
    nan_idx = np.array([3, 63, 64, K // 2, K - 2, K - 1])
    ctl = ctl.copy()
    ctl[nan_idx[0::2]] = NAN_A
    ctl[nan_idx[1::2]] = NAN_B
    assert np.unique(bits(ctl[nan_idx])).size == 2
    g = weighted(p, ctl, state, xr, yr, yaw0, lam)
    costs = g.read_costs()
    is_nan = np.zeros(K, dtype=bool)
    is_nan[nan_idx] = True
    np.testing.assert_array_equal(np.isnan(costs), is_nan)
    gc = np.sort(group_costs(costs, group, ~is_nan))
    host_w = np.exp(-(gc - gc[0]) / lam)
    assert np.all(host_w[1:] < host_w[:-1] * (1.0 - 1e-6))
    expected = np.concatenate([nan_idx, np.lexsort((np.arange(K), costs))[:K - nan_idx.size]])
    top_w = check_top_calls(g, expected, "nan K=%d %s" % (K, deal))
    assert np.all(np.isnan(top_w[:nan_idx.size])) and not np.any(np.isnan(top_w[nan_idx.size:]))
    print("K=%d %s: NaN weight patterns %s, NaN cost patterns %s" % (K, deal, sorted(hex(b) for b in np.unique(bits(top_w[:nan_idx.size]))),
                                                                    sorted(hex(b) for b in np.unique(bits(costs[nan_idx])))))
    g.close()


# ---- 3. the gathers ---------------------------------------------------------------------------------------------------------------
GATHER = [("diff_drive", 1000, 15), ("steering_diff_drive", 1000, 15), ("full_body", 1000, 15), ("diff_drive", 1025, 15),
          ("diff_drive", 1000, 16), ("diff_drive", 1000, 3)]


@pytest.fixture(scope="module")
def iterated():
    made = {}

    def get(model, K, H):
        if (model, K, H) not in made:
            p = MODEL_DEFAULTS[model](K, H).with_(lam=1000.0)   # (every sample carries weight: the weights tell the samples apart)
            path = helpers.oracle_path("sinusoid")
            state = np.zeros(p.nstate)
            state[0], state[1] = path[0][0], path[1][0] + 0.05
            xr, yr, yaw = helpers.oracle_window(p, path, state)
            g = MPPIController(p)
            g.iterate(state, p.dt, xr, yr, yaw[0], 17, 3, want_stats=False)
            made[(model, K, H)] = (g, g.read_candidates(), g.read_weights())
        return made[(model, K, H)]
    yield get
    for g, _, _ in made.values():
        g.close()


def gather_ranges(K, H):
    """(first, count, stride): the ends of the admitted range, a stride across it, strides that reach K - 1 and beyond it, and
    contiguous ranges whose count * H meets the 256 threads of a workgroup of k_gather_xy: 255, 256 and the first beyond (257 is
    prime and H is 3 .. 128, so no count * H equals it: 258 = 86 * 3 stands in, at H = 3)"""
    out = [(0, 1, 1), (K - 1, 1, 1), (K - 1, 1, 7), (0, K, 1), (3, (K - 4) // 5 + 1, 5), (0, 2, K - 1), (1, 1, K)]
    out += [(5, n // H, 1) for n in (255, 256, 258) if n % H == 0]
    return out


def raw_candidates(g, first, count, stride, rows):
    out = np.full((rows, g.H, 2), -7.0)
    return g.lib.ccv_mppi_read_candidates(g._h, int(first), int(count), int(stride), capi.dptr(out)), out


@pytest.mark.parametrize("model,K,H", GATHER)
def test_read_candidates_with_first_count_and_stride(iterated, model, K, H):
    g, full, _ = iterated(model, K, H)
    assert full.shape == (K, H, 2) and np.all(np.isfinite(full))
    assert np.unique(bits(full[:, -1, 0])).size > K // 2       # (the rows tell the samples apart)
    ranges = gather_ranges(K, H)
    assert {c * H for _, c, s in ranges if s == 1 and 1 < c < K} == {15: {255}, 16: {256}, 3: {255, 258}}[H]
    for first, count, stride in ranges:
        last = first + (count - 1) * stride
        assert last <= K - 1
        rc, out = raw_candidates(g, first, count, stride, count + 1)
        assert rc == capi.OK, (first, count, stride)
        same_bits(out[:count], full[first::stride][:count], "first=%d count=%d stride=%d" % (first, count, stride))
        assert np.all(out[count:] == -7.0)
        # ... the same range with its last index moved to K
        rc, out = raw_candidates(g, first + (K - last), count, stride, count + 1)
        assert rc == capi.ERR_INVALID_ARG and np.all(out == -7.0), (first + (K - last), count, stride)
    for first, count, stride in ((0, 1, 0), (0, K, 0), (-1, 1, 1), (0, -1, 1), (0, 1, -1), (K, 1, 1), (0, K + 1, 1), (1, 2, K - 1)):
        rc, out = raw_candidates(g, first, count, stride, 2)
        assert rc == capi.ERR_INVALID_ARG and np.all(out == -7.0), (first, count, stride)
    with pytest.raises(MPPIError):
        g.read_candidates(first=K - 1, count=2, stride=1)


@pytest.mark.parametrize("model,K,H", GATHER[:4])
def test_read_weights_with_first_and_count(iterated, model, K, H):
    g, _, wn = iterated(model, K, H)
    assert wn.shape == (K,)
    for i in (0, 254, 255, 256, K - 2):   # (a range shifted by one sample would show)
        assert bits(wn[i:i + 1])[0] != bits(wn[i + 1:i + 2])[0], "weights %d and %d are the same" % (i, i + 1)
    for first, count in ((0, 1), (K - 1, 1), (255, 2), (1, K - 1)):
        out = np.full(count + 1, -7.0)
        assert g.lib.ccv_mppi_read_weights(g._h, first, count, capi.dptr(out)) == capi.OK
        same_bits(out[:count], wn[first:first + count], "first=%d count=%d" % (first, count))
        assert out[count] == -7.0
    for first, count in ((K, 1), (1, K), (-1, 1), (0, -1)):
        out = np.full(2, -7.0)
        assert g.lib.ccv_mppi_read_weights(g._h, first, count, capi.dptr(out)) == capi.ERR_INVALID_ARG and np.all(out == -7.0)

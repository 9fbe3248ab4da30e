"""GPU tests (-m gpu) of the batch handles' feed calls (ccv_mppi_batch_read_best_candidates / _read_optimal_paths,
BatchController.read_best_candidates / read_optimal_paths).

Checkers: tests/select_reference.py (the order as numpy states it) for select_lowest() behind tests/probe/select_probe.hip and
for the call itself, over the costs ccv_mppi_batch_read_costs returns; ccv_mppi_batch_read_candidates for the gathered states;
ccv_mppi_plant_step on the host for the optimal paths.  Every comparison is of integers or of bit patterns: no tolerances.
"""
import ctypes as C

import numpy as np
import pytest

import ccv_mppi_path_tracker_amd as amd
import select_probe
import select_reference as R
from batch_support import MODEL_DEFAULTS, instance_seed, path_of
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIError

pytestmark = pytest.mark.gpu

MODELS = ("diff_drive", "steering_diff_drive", "full_body")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tick_inputs(p, B, salt=0, yaw_offset=None):
    """Distinct inputs per instance: a pose near its path, dt, window, seed, warm start."""
    x0, xr, yr = np.zeros((B, p.nstate)), np.zeros((B, p.horizon)), np.zeros((B, p.horizon))
    dt, yaw0, seeds = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.uint64)
    for b in range(B):
        px, py = path_of(b)
        i = (37 * b + 11 * salt + 5) % (len(px) // 2)
        x0[b, 0], x0[b, 1] = px[i], py[i] + 0.05 * ((b % 5) - 2)
        x0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        if yaw_offset is not None:
            x0[b, 2] += yaw_offset[b]
        if p.nstate == 5:
            x0[b, 3], x0[b, 4] = 0.02 * ((b % 3) - 1), -0.01 * (b % 2)
        dt[b] = p.dt * (1.0 + 0.05 * (b % 4))
        _, xr[b], yr[b], yaw = amd.calc_ref_path(px, py, x0[b, 0], x0[b, 1], p.v_ref, dt[b], p.resolution, p.horizon)
        yaw0[b] = yaw[0]
        seeds[b] = instance_seed(b, salt)
    lo, hi = np.array(p.u_min), np.array(p.u_max)
    rng = np.random.default_rng(99 + salt)
    nom = np.clip(0.3 * (hi - lo) / 2 * rng.standard_normal((B, p.horizon - 1, p.udim)) + (hi + lo) / 2, lo, hi)
    return x0, dt, xr, yr, yaw0, seeds, nom


def ticked(p, B, K, salt=0, nominal=None, setup=None, **kw):
    """a batch handle after one host-record tick, and that tick's inputs"""
    inp = tick_inputs(p if isinstance(p, configs.MPPIParams) else p[0], B, salt, kw.pop("yaw_offset", None))
    bat = BatchController(p, B, num_samples=K, **kw)
    if setup:
        setup(bat)
    bat.set_nominal(inp[6] if nominal is None else nominal)
    bat.iterate_enqueue(*inp[:6], 0)
    return bat, inp


def assert_best_is_the_lexsort(bat, count, paths=(0, None, -1)):
    """indices = the lexsort of read_costs, costs bit-equal, the rows of xy those of read_candidates; returns the arrays"""
    idx, cost, xy = bat.read_best_candidates(count)
    assert idx.shape == (bat.B, count) and idx.dtype == np.int32 and cost.shape == (bat.B, count) and xy.shape == (bat.B, count, bat.H, 2)
    for b in range(bat.B):
        costs = bat.read_costs(b)
        want, _ = R.lowest(costs, count)
        np.testing.assert_array_equal(idx[b], want)
        np.testing.assert_array_equal(bits(cost[b]), bits(costs[want]))
        for j in {(count // 2 if j is None else j) % count for j in paths}:
            np.testing.assert_array_equal(bits(xy[b, j]), bits(bat.read_candidates(b, first=int(idx[b, j]), count=1)[0]))
    return idx, cost, xy


# ---- 1. select_lowest() behind the probe, against the numpy reference -------------------------------------------------------
PROBE_K = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
SPECIALS = np.concatenate([np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e308, -1e308]),
                           np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF],
                                    dtype=np.uint64).view(np.float64)])


def counts_for(K):
    return sorted({n for n in (1, 2, 63, 64, 65, K, min(K, 1024)) if n <= K and n <= capi.BEST_MAX})


def one_byte_varies(K, digit, seg):
    """doubles whose keys differ in radix digit `digit` only (K > 256: in runs of equal values); no NaN among them"""
    words = np.full(K, 0x4010203040506070, dtype=np.uint64) & ~np.uint64(0xFF << (8 * digit))
    return (words | (((np.arange(K, dtype=np.uint64) * np.uint64(7 + 2 * seg)) & np.uint64(0xFF)) << np.uint64(8 * digit))).view(np.float64)


def probe_inputs(K, rng):
    """{name: [3 segments of K doubles]}; the inputs that depend on the count N are made in the test"""
    out = {"random": [rng.standard_normal(K) * 10.0 ** rng.integers(-5, 6) for _ in range(3)],
           "all_equal": [np.full(K, v) for v in (3.25, -7.0, np.inf)],
           "nan_finite_inf": [SPECIALS[rng.integers(0, SPECIALS.size, size=K)] for _ in range(3)],
           "zeros": [np.where(rng.integers(0, 2, size=K) == 0, 0.0, -0.0), np.full(K, -0.0),
                     np.where(rng.integers(0, 3, size=K) == 0, -1.0, np.where(rng.integers(0, 2, size=K) == 0, 0.0, -0.0))]}
    for digit in range(8):   # (digit 0: the lowest byte; digit 7: the highest, sign and exponent)
        out["digit%d" % digit] = [one_byte_varies(K, digit, s) for s in range(3)]
    return out


@pytest.mark.parametrize("K", PROBE_K)
def test_select_lowest_is_the_reference_order(K):
    rng = np.random.default_rng(1000 + K)
    pitch = (K + 63) // 64 * 64 + 64   # (padding even where K is a multiple of 64)
    inputs = probe_inputs(K, rng)
    for N in counts_for(K):
        # two distinct values, the N-th place inside the run of the higher ones: N // 2 low ones at random places
        inputs["two_values"] = []
        for s in range(3):
            c = np.full(K, 2.5)
            c[rng.permutation(K)[:N // 2]] = -1.5 - s
            inputs["two_values"].append(c)
        for name, segs in inputs.items():
            grid = np.full((3, pitch), -np.inf)   # (the padding would win if it were read)
            for s in range(3):
                grid[s, :K] = segs[s]
            idx, key = select_probe.lowest(grid, K, N)
            for s in range(3):
                want_idx, want_key = R.lowest(segs[s], N)
                np.testing.assert_array_equal(idx[s], want_idx, err_msg="%s K=%d N=%d segment %d" % (name, K, N, s))
                np.testing.assert_array_equal(key[s], want_key, err_msg="%s K=%d N=%d segment %d" % (name, K, N, s))


# ---- 2. through the ABI, host-record tick -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_ticks():
    made = {}

    def get(model):
        if model not in made:
            made[model] = ticked(MODEL_DEFAULTS[model](1000, 15), 3, 1000)[0]
        return made[model]
    yield get
    for bat in made.values():
        bat.close()


@pytest.mark.parametrize("count", (1, 7, 1000))
@pytest.mark.parametrize("model", MODELS)
def test_best_candidates_of_a_host_record_tick(host_ticks, model, count):
    bat = host_ticks(model)
    idx, cost, xy = assert_best_is_the_lexsort(bat, count)
    if count == bat.K:   # (the padding columns 1000 .. 1023 are never selected)
        np.testing.assert_array_equal(np.sort(idx, axis=1), np.tile(np.arange(bat.K, dtype=np.int32), (bat.B, 1)))
    again = bat.read_best_candidates(count)
    for a, b in zip((idx, bits(cost), bits(xy)), (again[0], bits(again[1]), bits(again[2]))):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("K", (64, 65))
def test_best_candidates_at_the_edge_of_a_workgroup(K):
    bat, _ = ticked(configs.diff_drive_defaults(K, 15), 3, K, salt=K)
    for count in (1, 7, K):
        idx, _, _ = assert_best_is_the_lexsort(bat, count)
    np.testing.assert_array_equal(np.sort(idx, axis=1), np.tile(np.arange(K, dtype=np.int32), (3, 1)))
    bat.close()


# ---- 3. kernel families and forms ---------------------------------------------------------------------------------------------
def test_best_candidates_after_the_plain_kernel(monkeypatch):
    monkeypatch.setenv("CCV_MPPI_KERNEL", "v1")
    bat, _ = ticked(configs.diff_drive_defaults(1000, 15), 3, 1000, salt=1)
    monkeypatch.delenv("CCV_MPPI_KERNEL")
    assert bat.last_kernel() == capi.BATCH_KERNEL_PLAIN
    assert_best_is_the_lexsort(bat, 7)
    bat.close()


def test_best_candidates_after_the_one_wave_kernel():
    bat, _ = ticked(configs.diff_drive_defaults(1000, 15), 81, 1000, salt=2)
    assert bat.last_kernel() == capi.BATCH_KERNEL_ONE_WAVE
    assert_best_is_the_lexsort(bat, 7)
    bat.close()


def test_best_candidates_under_shifted_weights():
    bat, _ = ticked(configs.diff_drive_defaults(1000, 15), 3, 1000, salt=3, min_shift=True)
    assert bat.last_kernel() & capi.BATCH_KERNEL_SHIFT
    assert_best_is_the_lexsort(bat, 7)
    bat.close()


def test_best_candidates_with_per_instance_params_and_discs():
    p = configs.diff_drive_defaults(1000, 15)
    seq = [p.with_(lam=0.5 + b, control_noise=0.3 + 0.2 * b, v_ref=0.6 + 0.1 * b) for b in range(3)]

    def setup(bat):
        bat.set_obstacles([[(1.0, 0.2, 0.5)], [], [(0.5, -0.1, 0.3), (2.0, 1.0, 0.4)]], weight=[3.0, 0.0, 5.0])
    bat, _ = ticked(seq, 3, 1000, salt=4, setup=setup)
    assert bat.last_kernel() & capi.BATCH_KERNEL_OBST and bat.last_kernel() & capi.BATCH_KERNEL_VARIED
    assert_best_is_the_lexsort(bat, 7)
    bat.close()


# ---- 4. ties and NaN without a probe ------------------------------------------------------------------------------------------
def test_equal_costs_and_nan_costs_come_out_by_index():
    p = configs.diff_drive_defaults(1000, 15)
    pinned = (0.7, 0.4)   # (not zero: a sample of -0.0 would pass a clamp to +0.0 unchanged)
    seq = [p.with_(u_min=pinned, u_max=pinned), p, p]   # instance 0: every sample clamps to the same controls
    nom = tick_inputs(p, 3, 5)[6]
    nom[1, 0, 0] = np.nan                                 # instance 1: a NaN speed in the warm start, every cost NaN
    bat, _ = ticked(seq, 3, 1000, salt=5, nominal=nom)
    c0, c1 = bat.read_costs(0), bat.read_costs(1)
    assert np.all(bits(c0) == bits(c0)[0]) and np.all(np.isnan(c1))
    for count in (1, 7, 1000):
        idx, cost, _ = assert_best_is_the_lexsort(bat, count)   # (instance 2: its own lexsort)
        np.testing.assert_array_equal(idx[0], np.arange(count))
        np.testing.assert_array_equal(idx[1], np.arange(count))
        assert np.all(np.isnan(cost[1]))
    bat.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    p = configs.diff_drive_defaults(256, 15)
    bat = BatchController(p, 2)
    lib, i32p = bat.lib, C.POINTER(C.c_int32)
    idx, cost, xy, path = np.zeros((2, 4), dtype=np.int32), np.zeros((2, 4)), np.zeros((2, 4, 15, 2)), np.zeros((2, 14, 3))
    for call in (lambda: bat.read_best_candidates(4), bat.read_optimal_paths):
        with pytest.raises(MPPIError) as ei:   # before any tick
            call()
        assert ei.value.code == capi.ERR_STATE
    x0, dt, xr, yr, yaw0, seeds, nom = tick_inputs(p, 2)
    bat.iterate_enqueue(x0, dt, xr, yr, yaw0, seeds, 0)
    for count in (-1, 257, 1025):
        with pytest.raises(MPPIError) as ei:
            bat.read_best_candidates(count)
        assert ei.value.code == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_best_candidates(bat._h, 4, None, capi.dptr(cost), capi.dptr(xy)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_optimal_paths(bat._h, None) == capi.ERR_INVALID_ARG
    untouched = idx.copy()
    assert lib.ccv_mppi_batch_read_best_candidates(bat._h, 0, idx.ctypes.data_as(i32p), None, None) == capi.OK   # writes nothing
    np.testing.assert_array_equal(idx, untouched)
    assert lib.ccv_mppi_batch_read_best_candidates(bat._h, 4, idx.ctypes.data_as(i32p), None, None) == capi.OK   # both may be null
    np.testing.assert_array_equal(idx, bat.read_best_candidates(4)[0])
    assert lib.ccv_mppi_batch_read_optimal_paths(bat._h, capi.dptr(path)) == capi.OK
    bat.close()
    big = BatchController(configs.diff_drive_defaults(1100, 15), 1)
    b_in = tick_inputs(big.params, 1)
    big.iterate_enqueue(*b_in[:6], 0)
    with pytest.raises(MPPIError) as ei:   # (within K, above the limit)
        big.read_best_candidates(1025)
    assert ei.value.code == capi.ERR_INVALID_ARG
    assert big.read_best_candidates(1024)[0].shape == (1, 1024)
    big.close()
    lean = BatchController(p, 2, no_state_store=True)
    lean.iterate_enqueue(x0, dt, xr, yr, yaw0, seeds, 0)
    with pytest.raises(MPPIError) as ei:
        lean.read_best_candidates(4)
    assert ei.value.code == capi.ERR_STATE
    got, gcost, none = lean.read_best_candidates(4, with_paths=False)
    assert none is None
    for b in range(2):
        want, _ = R.lowest(lean.read_costs(b), 4)
        np.testing.assert_array_equal(got[b], want)
    lean.close()


# ---- 6. the resident loop is not disturbed ------------------------------------------------------------------------------------
def start_poses(p, B):
    x0, _, _, _, _, seeds, _ = tick_inputs(p, B, salt=6)
    return x0, seeds


def end_state(bat):
    st, idx, xr, yr, yaw0, steps = bat.resident_read()
    return [st, idx, xr, yr, yaw0, np.array(steps), bat.get_nominal()] + [bat.resident_read_trace(b) for b in range(bat.B)]


@pytest.mark.parametrize("model", ("diff_drive", "full_body"))
def test_the_feed_leaves_a_resident_loop_bit_for_bit(model):
    p, B, ticks = MODEL_DEFAULTS[model](256, 15), 4, 6
    s0, seeds = start_poses(p, B)
    ends = []
    for feed in ("none", "best", "best+paths"):
        bat = BatchController(p, B)
        bat.resident_set_paths([path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, seeds)
        bat.resident_set_fleet([0.3, 0.0, 0.0, 0.0], 5.0, 2, 1.0)
        for it in range(ticks):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            if feed != "none":
                idx, cost, xy = bat.read_best_candidates(5)
                assert np.all((idx >= 0) & (idx < bat.K)) and np.all(cost[:, 1:] >= cost[:, :-1])
            if feed == "best+paths":
                assert bat.read_optimal_paths().shape == (B, p.horizon - 1, 3)
        if feed == "best":   # (after the last tick, before anything flushes: the call against the plain read-backs)
            idx, cost, xy = bat.read_best_candidates(5)
            for b in range(B):
                want, _ = R.lowest(bat.read_costs(b), 5)
                np.testing.assert_array_equal(idx[b], want)
                np.testing.assert_array_equal(bits(xy[b, 0]), bits(bat.read_candidates(b, first=int(idx[b, 0]), count=1)[0]))
        ends.append(end_state(bat))
        bat.close()
    for other in ends[1:]:
        for a, b in zip(ends[0], other):
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


# ---- 7. optimal paths ---------------------------------------------------------------------------------------------------------
def host_paths(p, poses, u, dt):
    """H - 1 ccv_mppi_plant_step calls per instance: row i = (x, y, yaw) before control step i"""
    B = poses.shape[0]
    out = np.zeros((B, p.horizon - 1, 3))
    for b in range(B):
        s = np.array(poses[b], dtype=np.float64)
        for i in range(p.horizon - 1):
            out[b, i] = s[:3]
            s = amd.plant_step(p.model, s, u[b, i], float(dt[b]))
    return out


@pytest.mark.parametrize("model", MODELS)
def test_optimal_paths_are_the_host_plant_bit_for_bit(model):
    p, B = MODEL_DEFAULTS[model](256, 15), 4
    # host-record tick; instance 1 starts at a heading of 9e4 rad (inside the sin / cos range, rebased by the first step),
    # instance 2 just beyond 1e4, where the rebase acts as well.  Full body charges the heading against yaw_ref: at 9e4 rad every
    # plain weight underflows and u* is NaN, which the host plant refuses -- it runs with the underflow-safe weights.
    shift = model == "full_body"
    bat, (x0, dt, xr, yr, yaw0, seeds, nom) = ticked(p, B, 256, salt=7, yaw_offset=[0.0, 9.0e4, 1.2e4, 0.0], min_shift=shift)
    got = bat.read_optimal_paths()
    u = bat.get_nominal()
    assert not np.array_equal(u, nom) and np.all(np.isfinite(u))
    np.testing.assert_array_equal(bits(got), bits(host_paths(p, x0, u, dt)))
    assert abs(got[1, 0, 2]) > 8.0e4 and abs(got[1, 1, 2]) < 4.0 and abs(got[2, 0, 2]) > 1.0e4 and abs(got[2, 1, 2]) < 4.0
    bat.close()
    # resident ticks: the pose and dt are the prologue's
    bat = BatchController(p, B, min_shift=shift)
    s0, seeds = start_poses(p, B)
    s0[3, 2] += 1.2e4
    bat.resident_set_paths([path_of(b) for b in range(B)])
    bat.resident_set_poses(s0, seeds)
    for it in range(3):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        if it in (0, 2):
            got = bat.read_optimal_paths()
            poses = bat.resident_read()[0]
            np.testing.assert_array_equal(bits(got), bits(host_paths(p, poses, bat.get_nominal(), np.full(B, p.dt))))
            np.testing.assert_array_equal(bits(got[:, 0, :]), bits(poses[:, :3]))
    bat.close()

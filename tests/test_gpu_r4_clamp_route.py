"""GPU tests (-m gpu): the four-wave rollout kernel's two clamp routes against kernel families that have one route only.

The dynamics wave of k_rollout_r4 (csrc/mppi_rollout_r4.h) runs its time blocks with the two-instruction clamp when the host has
vouched for sigma and the bounds and the staging found no NaN in the warm start, and with the reference's compare-and-select clamp
otherwise; for diff drive and steering each route is a loop of its own, chosen once per launch.  Whatever the route, the results are
to be the bits of the families that clamp by compare-and-select throughout: the three-wave kernel (CCV_MPPI_KERNEL=r3), which shares
the batched producer, in every quantity -- stored normals (read back as controls), x / y states, costs, weights, u* after the update;
NaNs in the same places -- and the plain kernel (v1) in the controls.  v1 evaluates sin / cos with the device library where the
multi-wave kernels advance or evaluate them branch-free, so its states, costs, weights and u* are not the same bits for ANY launch
(test_kernel_variants_agree holds them at rtol 1e-13 / 1e-12 / 1e-10): those are held at these tolerances here, with NaNs
in the same places.  The wide-turn case (|w|max dt > pi/4): r3 and v1 are routed to the plain kernel there (fast_trig_safe), and
the one family with a wide form of its own is the one-wave kernel (solo), whose samples and states are the four-wave kernel's bits
(test_gpu_horizon_sweep.py); costs and u* differ by the order in which the cost parts are added (rtol 1e-12 / 1e-10, as
test_one_wave_kernel_agrees_with_the_multi_wave_kernels).

K = 200: three full workgroups and one with 8 live lanes.  H = 9, 10, 15, 17, 50: no tail, a one-step tail, the six-step TAIL form,
a one-step tail after two full blocks, C2's horizon.  Routes: healthy; healthy with the host's consent withdrawn
(CCV_MPPI_FAST_CLAMP=0); a NaN in control row 0, in the last row of block 0, in the first row of block 1, in the last control row,
and in two rows at once.  Every four-wave run twice: wave priorities on and off (CCV_MPPI_PRIO=0).
"""
import numpy as np
import pytest

import helpers
from batch_support import MODEL_DEFAULTS, close_all, instance_inputs
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController

pytestmark = pytest.mark.gpu

K = 200
HORIZONS = (9, 10, 15, 17, 50)
SEED, IT = 13, 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def nan_rows(route, H, udim):
    """(row, control dimension) of the NaNs of a route; None: the horizon has no such row."""
    last = H - 2
    return {"healthy": [], "host_off": [],
            "nan_row0": [(0, 0)],
            "nan_end_block0": [(min(7, last), 1)],
            "nan_start_block1": [(8, 0)] if last >= 8 else None,
            "nan_last_row": [(last, udim - 1)],
            "nan_two_rows": [(1, 1), (last, 0)]}[route]


ROUTES = ("healthy", "host_off", "nan_row0", "nan_end_block0", "nan_start_block1", "nan_last_row", "nan_two_rows")
CASES = [(wl, H, r) for wl in ("C2", "C3") for H in HORIZONS for r in ROUTES
         if nan_rows(r, H, configs.workload(wl).params.udim) is not None]


def setup(wl, H, **over):
    w = configs.workload(wl)
    p = w.params.with_(num_samples=K, horizon=H, **over)
    path = helpers.oracle_path(w.path)
    state = np.zeros(p.nstate)
    state[0], state[1] = path[0][0], path[1][0] - 0.1
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    return p, state, xr, yr, yaw[0]


def warm_start(p, rows):
    """A warm start that reaches both bounds in places (so both clamps bite), NaN at `rows`."""
    lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
    rng = np.random.default_rng(p.horizon)
    nom = np.clip((hi + lo) / 2 + 0.45 * (hi - lo) * rng.standard_normal((p.horizon - 1, p.udim)), lo, hi)
    for t, d in rows:
        nom[t, d] = np.nan
    return nom


def run(monkeypatch, p, state, xr, yr, yaw0, nom, kernel, prio=None, iters=1):
    """A fresh handle of one family; what each of `iters` iterations from the warm start leaves behind."""
    monkeypatch.setenv("CCV_MPPI_KERNEL", kernel)
    if prio is None:
        monkeypatch.delenv("CCV_MPPI_PRIO", raising=False)
    else:
        monkeypatch.setenv("CCV_MPPI_PRIO", prio)
    g = MPPIController(p)
    g.set_nominal(nom)
    out = []
    for it in range(iters):
        u = g.iterate(state, p.dt, xr, yr, yaw0, SEED, IT + it, want_stats=False)
        out.append(dict(ctl=g.read_controls(), xy=g.read_candidates(), cost=g.read_costs(), w=g.read_weights(), u=np.array(u)))
    g.close()
    return out


def same_bits(what, a, b, keys=("ctl", "xy", "cost", "w", "u")):
    """Bit patterns equal wherever a value is not NaN, NaNs in the same places."""
    for k in keys:
        x, y = np.ascontiguousarray(a[k], dtype=np.float64), np.ascontiguousarray(b[k], dtype=np.float64)
        assert x.shape == y.shape, (what, k)
        nx, ny = np.isnan(x), np.isnan(y)
        assert np.array_equal(nx, ny), f"{what}: {k}: NaNs in other places ({nx.sum()} / {ny.sum()})"
        bx, by = x.view(np.uint64)[~nx], y.view(np.uint64)[~ny]
        assert np.array_equal(bx, by), f"{what}: {k}: {np.count_nonzero(bx != by)} of {bx.size} values differ in their bits"


def close_to(what, a, b, tol):
    """NaNs in the same places (assert_allclose holds that too), finite values within the named test's tolerances."""
    for k, (rtol, atol) in tol.items():
        np.testing.assert_allclose(a[k], b[k], rtol=rtol, atol=atol, err_msg=f"{what}: {k}")


# (test_kernel_variants_agree; the weights exp(-cost / lambda) at test_injected_controls_match_oracle's rtol 1e-8)
TOL_PLAIN = {"xy": (1e-13, 1e-13), "cost": (1e-12, 0.0), "w": (1e-8, 1e-300), "u": (1e-10, 1e-14)}
# (test_one_wave_kernel_agrees_with_the_multi_wave_kernels)
TOL_ORDER = {"cost": (1e-12, 0.0), "w": (1e-8, 1e-300), "u": (1e-10, 1e-13)}


@pytest.mark.parametrize("wl,H,route", CASES)
def test_both_routes_give_the_other_families_bits(monkeypatch, wl, H, route):
    p, state, xr, yr, yaw0 = setup(wl, H)
    rows = nan_rows(route, H, p.udim)
    nom = warm_start(p, rows)
    if route == "host_off":
        monkeypatch.setenv("CCV_MPPI_FAST_CLAMP", "0")
    else:
        monkeypatch.delenv("CCV_MPPI_FAST_CLAMP", raising=False)
    iters = 1 if rows else 2   # (healthy: the second iteration starts from the first one's update)
    args = (monkeypatch, p, state, xr, yr, yaw0, nom)
    r4s, r4s_flat, r3s = run(*args, "r4", iters=iters), run(*args, "r4", prio="0", iters=iters), run(*args, "r3", iters=iters)
    v1 = run(*args, "v1")[0]   # (the first iteration: after it the warm starts differ by the update's rounding)
    r4 = r4s[0]
    # the NaNs are where the reference puts them: every control of a NaN row's dimension, nowhere else; a clamp bites somewhere
    expect_nan = np.zeros(r4["ctl"].shape, dtype=bool)
    for t, d in rows:
        expect_nan[:, t, d] = True
    assert np.array_equal(np.isnan(r4["ctl"]), expect_nan)
    lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
    assert ((r4["ctl"] == lo) | (r4["ctl"] == hi)).any()
    if rows:
        assert all(np.isnan(r4["u"][t, d]) for t, d in rows)   # (a weighted mean of NaN controls)
    else:
        assert np.all(np.isfinite(r4["u"])) and np.all(np.isfinite(r4["cost"]))
    for it in range(iters):
        same_bits(f"priorities on / off, iteration {it}", r4s[it], r4s_flat[it])
        same_bits(f"r4 / r3, iteration {it}", r4s[it], r3s[it])
    same_bits("r4 / v1", r4, v1, keys=("ctl",))
    close_to("r4 / v1", r4, v1, TOL_PLAIN)


@pytest.mark.parametrize("route", ["healthy", "nan_row0", "nan_start_block1", "nan_last_row"])
def test_wide_turn_form_on_both_routes(monkeypatch, route):
    """dt = 0.4: |w|max dt > pi/4, the WIDE instantiation (one-step tail at H = 18, two full blocks before it)."""
    H = 18
    p, state, xr, yr, yaw0 = setup("C2", H, dt=0.4)
    assert max(abs(p.u_min[1]), abs(p.u_max[1])) * p.dt > np.pi / 4
    rows = nan_rows(route, H, p.udim)
    nom = warm_start(p, rows)
    monkeypatch.delenv("CCV_MPPI_FAST_CLAMP", raising=False)
    args = (monkeypatch, p, state, xr, yr, yaw0, nom)
    r4, r4_flat, solo = run(*args, "r4")[0], run(*args, "r4", prio="0")[0], run(*args, "solo")[0]
    r3, v1 = run(*args, "r3")[0], run(*args, "v1")[0]   # (both the plain kernel here)
    same_bits("priorities on / off", r4, r4_flat)
    same_bits("r4 / solo (wide)", r4, solo, keys=("ctl", "xy"))
    close_to("r4 / solo (wide)", r4, solo, TOL_ORDER)
    for name, other in (("r3", r3), ("v1", v1)):
        same_bits("r4 / plain kernel as " + name, r4, other, keys=("ctl",))
        close_to("r4 / plain kernel as " + name, r4, other, TOL_PLAIN)
    assert all(np.isnan(r4["u"][t, d]) for t, d in rows) and (rows or np.all(np.isfinite(r4["u"])))


@pytest.mark.parametrize("model", ["diff_drive", "steering_diff_drive"])
def test_batch_instances_take_their_own_route(monkeypatch, model):
    """B = 3, H = 15 (the TAIL form of the batch kernels): instance 0 healthy, 1 with a NaN in block 0, 2 with a NaN in the masked
    last block -- every instance equal to a single handle from the same warm start, bit for bit."""
    monkeypatch.delenv("CCV_MPPI_KERNEL", raising=False)
    monkeypatch.delenv("CCV_MPPI_PRIO", raising=False)
    monkeypatch.delenv("CCV_MPPI_FAST_CLAMP", raising=False)
    B, H = 3, 15
    p = MODEL_DEFAULTS[model](K, H)
    x0, dt, xr, yr, yaw0, seeds, nom = instance_inputs(p, B)
    nom[1, 3, 1] = np.nan
    nom[2, H - 2, 0] = np.nan
    bat = BatchController(p, B)
    bat.set_nominal(nom)
    ub, _ = bat.iterate(x0, dt, xr, yr, yaw0, seeds, IT)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE
    singles = []
    for b in range(B):
        g = MPPIController(p)
        singles.append(g)
        g.set_nominal(nom[b])
        us = g.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], int(seeds[b]), IT, want_stats=False)
        one = dict(xy=g.read_candidates(), cost=g.read_costs(), w=g.read_weights(), u=np.array(us))
        many = dict(xy=bat.read_candidates(b), cost=bat.read_costs(b), w=bat.read_weights(b), u=ub[b])
        same_bits(f"batch instance {b} / single handle", many, one, keys=("xy", "cost", "w", "u"))
        assert np.isnan(one["u"]).any() == (b > 0)
    close_all(bat, *singles)

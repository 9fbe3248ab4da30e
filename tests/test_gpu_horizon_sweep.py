"""GPU tests (-m gpu): every horizon H = 3 .. 26 through every rollout kernel family of the single handle, against the oracle.

Every rollout kernel cuts the horizon into blocks of eight steps and treats the last block by H (tests/horizon_cases.py restates
the arithmetic, tests/test_horizon_cases_cpu.py proves what these horizons reach): a full batch, the masked PARTIAL batch from four
control steps on (the four-wave kernel: a TAIL instantiation of its own, and one more for six steps), step by step below; one of
eight pc_consume<nv> on the distance side; pruning from H = 17 on; and for H = 5 .. 8 block 0 is itself the partial block.  The
other suites run fifteen horizons between them; here one model row x one horizon is one test, K = 130 (three workgroups, two live
lanes in the last), the dkan path with a lateral offset, two iterations (the second from the first one's update, the oracle put on
the device's nominal).

No tolerance is new.  Each comparison takes the one of the test that makes it at its few horizons:
  * controls bit-equal to the oracle's Philox samples; states rtol 1e-12, atol 1e-13 (test_injected_controls_match_oracle);
    costs < TOL_COST; u* < 1e-9 (iteration 0) and < 1e-8 (iteration 1); sum_w within 1e-9 (test_horizon_extremes,
    test_fused_iteration_matches_oracle_philox) -- for every handle: the default family, CCV_MPPI_KERNEL = r4, r3 (not full
    body), pc, solo, v1, and the stage-wise twins (sampling / predict_States / calc_Weights / determine_OptimalSolution) of the
    default, r3 and pc handles;
  * r3 == the default four-wave handle in every bit -- samples, states, costs, weights, u* (test_multi_wave_kernels_agree);
  * fused == stage-wise in every bit for the same family (test_fused_equals_stagewise_bitwise);
  * iteration 0: samples and states bit-equal across r4, r3, pc and solo (the docstrings of the three agreement tests);
  * CCV_MPPI_FAST_CLAMP=0 on r4 and solo (test_forced_clamp_*): controls the oracle's bits with bounds that bite, u* at TOL_U,
    and against the fast twin as test_two_instruction_clamp_equals_compare_and_select.

The dt = 0.4 row (|w|max dt > pi/4).  Only the fused four-wave and one-wave kernels have a wide-turn form (has_wide_form,
csrc/capi_internal.h); every other launch of that row -- r3, pc, v1, every stage-wise call -- is routed to the plain kernel
(fast_trig_safe).  So in that row the forced r4 handle equals the default in every bit, the samples are the oracle's bits
everywhere, and everything else is held against the oracle alone: the family names of that row say how the handle was created,
not which kernel ran.
"""
import numpy as np
import pytest

import helpers
import horizon_cases as HC
from ccv_mppi_path_tracker_amd import capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController

pytestmark = pytest.mark.gpu

TOL_U = 1e-5      # as test_gpu_parity.py
TOL_COST = 1e-9
K = 130
SEED, IT0 = 2, 1
MAKERS = {"diff_drive": configs.diff_drive_defaults, "steering_diff_drive": configs.steering_defaults,
          "full_body": configs.full_body_defaults}
ROWS = {"dd": ("diff_drive", {}), "dd_wide": ("diff_drive", {"dt": 0.4}), "sd": ("steering_diff_drive", {}), "fb": ("full_body", {})}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def setup(row, H, **over):
    model, row_over = ROWS[row]
    p = MAKERS[model](K, H).with_(**dict(row_over, **over))
    path = helpers.oracle_path("dkan")
    state = np.zeros(p.nstate)
    state[0], state[1] = path[0][0], path[1][0] - 0.1
    xr, yr, yaw = helpers.oracle_window(p, path, state)
    return p, state, xr, yr, yaw[0]


def create(monkeypatch, p, kernel=None, fast_clamp=None):
    for name, value in (("CCV_MPPI_KERNEL", kernel), ("CCV_MPPI_FAST_CLAMP", fast_clamp)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    g = MPPIController(p)   # (both variables are read at create)
    monkeypatch.delenv("CCV_MPPI_KERNEL", raising=False)
    monkeypatch.delenv("CCV_MPPI_FAST_CLAMP", raising=False)
    return g


class OracleRuns:
    """the oracle's iteration from a given nominal, computed once per distinct nominal"""

    def __init__(self, p, state, xr, yr, yaw0):
        self.p, self.args, self.o, self.seen = p, (state, p.dt, xr, yr, yaw0), helpers.oracle_for(p), {}

    def run(self, nominal, it):
        key = (it, np.ascontiguousarray(nominal).tobytes())
        if key not in self.seen:
            o = self.o
            o.set_nominal(nominal)
            u = o.iterate(*self.args, seed=SEED, rng="philox", iteration=it)
            self.seen[key] = dict(u=np.array(u), ctl=np.array(o.get_controls()), x=np.array(o.states("x")), y=np.array(o.states("y")),
                                  c=np.array(o.costs()), sum_w=float(o.sum_w()))
        return self.seen[key]


def step(g, args, it, stagewise):
    """one iteration of handle g -> its read-backs"""
    state, dt, xr, yr, yaw0 = args
    if stagewise:
        g.sampling(SEED, it)
        g.predict_States(state, dt)
        g.calc_Weights(xr, yr, yaw0)
        u, st = g.determine_OptimalSolution(want_stats=True)
    else:
        u, st = g.iterate(state, dt, xr, yr, yaw0, SEED, it)
    return dict(u=np.array(u), sum_w=st.sum_w, ctl=g.read_controls(), xy=g.read_candidates(), c=g.read_costs(), w=g.read_weights())


def check_oracle(what, got, ref, tol_u, log):
    np.testing.assert_array_equal(got["ctl"], ref["ctl"], err_msg=what)
    np.testing.assert_allclose(got["xy"][..., 0], ref["x"], rtol=1e-12, atol=1e-13, err_msg=what)
    np.testing.assert_allclose(got["xy"][..., 1], ref["y"], rtol=1e-12, atol=1e-13, err_msg=what)
    ec = float(np.max(np.abs(got["c"] - ref["c"]) / np.maximum(np.abs(ref["c"]), 1e-300)))
    eu = helpers.rel_err(got["u"], ref["u"])
    es = abs(got["sum_w"] - ref["sum_w"]) / ref["sum_w"]
    log.append((what, ec / TOL_COST, eu / tol_u, es / 1e-9))
    assert ec < TOL_COST, (what, ec)
    assert eu < tol_u, (what, eu)
    assert es <= 1e-9, (what, es)


def same_bits(what, a, b, keys=("ctl", "xy", "c", "w", "u")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))
    if "u" in keys:
        assert a["sum_w"] == b["sum_w"], what


@pytest.mark.parametrize("H", HC.SINGLE_H)
@pytest.mark.parametrize("row", sorted(ROWS))
def test_every_family_matches_the_oracle(monkeypatch, row, H):
    p, state, xr, yr, yaw0 = setup(row, H)
    args = (state, p.dt, xr, yr, yaw0)
    fb, wide = p.model == "full_body", row == "dd_wide"
    # (name, CCV_MPPI_KERNEL, stage-wise)
    plan = [("default", None, False), ("r4", "r4", False), ("pc", "pc", False), ("solo", "solo", False), ("v1", "v1", False),
            ("default_stage", None, True), ("pc_stage", "pc", True)]
    if not fb:
        plan += [("r3", "r3", False), ("r3_stage", "r3", True)]
    handles = {name: (create(monkeypatch, p, kernel), stage) for name, kernel, stage in plan}
    oracle = OracleRuns(p, state, xr, yr, yaw0)
    log = []
    nominal = {name: np.zeros((H - 1, p.udim)) for name in handles}
    for i, it in enumerate((IT0, IT0 + 1)):
        got = {name: step(g, args, it, stage) for name, (g, stage) in handles.items()}
        for name, r in got.items():
            check_oracle("%s H=%d %s it%d" % (row, H, name, i), r, oracle.run(nominal[name], it), 1e-9 if i == 0 else 1e-8, log)
            nominal[name] = r["u"]
        same_bits("default == r4 forced", got["default"], got["r4"])
        if wide:   # (module docstring; the two families with a WIDE form meet here)
            if i == 0:
                same_bits("samples and states r4 / solo (wide)", got["r4"], got["solo"], keys=("ctl", "xy"))
        else:
            same_bits("default fused == stage-wise", got["default"], got["default_stage"])
            same_bits("pc fused == stage-wise", got["pc"], got["pc_stage"])
            if not fb:
                same_bits("r3 == default", got["default"], got["r3"])
                same_bits("r3 fused == stage-wise", got["r3"], got["r3_stage"])
            if i == 0:
                for name in ("pc", "solo") + (() if fb else ("r3",)):
                    same_bits("samples and states r4 / %s" % name, got["r4"], got[name], keys=("ctl", "xy"))
    worst = np.max(np.array([r[1:] for r in log]), axis=0)
    print("err/tol [horizon sweep] %s H=%d %s: costs %.3g  u* %.3g  sum_w %.3g" % (row, H, HC.block_shape(p.model, H), *worst))
    for g, _ in handles.values():
        g.close()


@pytest.mark.parametrize("H", HC.SINGLE_H)
@pytest.mark.parametrize("row", sorted(ROWS))
def test_forced_clamp_matches_the_oracle_and_its_fast_twin(monkeypatch, row, H):
    """CCV_MPPI_FAST_CLAMP=0 on the four-wave and the one-wave kernel: the PARTIAL instantiations of the compare-and-select
    clamp.  Wide noise, as test_two_instruction_clamp_equals_compare_and_select: many samples at a bound."""
    p, state, xr, yr, yaw0 = setup(row, H, control_noise=1.5)
    args = (state, p.dt, xr, yr, yaw0)
    oracle = OracleRuns(p, state, xr, yr, yaw0)
    lo, hi = np.array(p.u_min[:p.udim]), np.array(p.u_max[:p.udim])
    for kernel in ("r4", "solo"):
        fast, forced = create(monkeypatch, p, kernel), create(monkeypatch, p, kernel, fast_clamp="0")
        nominal = np.zeros((H - 1, p.udim))
        for i, it in enumerate((IT0, IT0 + 1)):
            a, b = step(fast, args, it, False), step(forced, args, it, False)
            what = "%s H=%d %s forced clamp it%d" % (row, H, kernel, i)
            ref = oracle.run(nominal, it)
            np.testing.assert_array_equal(b["ctl"], ref["ctl"], err_msg=what)
            np.testing.assert_allclose(b["u"], ref["u"], rtol=TOL_U, atol=1e-12, err_msg=what)
            assert np.max(np.abs(b["c"] - ref["c"]) / np.maximum(np.abs(ref["c"]), 1e-300)) < TOL_COST, what
            # (the twins start every iteration from the same nominal: the fast one is put on the forced one's below)
            np.testing.assert_array_equal(a["ctl"], b["ctl"], err_msg=what)
            assert np.mean((a["ctl"] == lo) | (a["ctl"] == hi)) > 0.05 and np.all(a["ctl"] >= lo) and np.all(a["ctl"] <= hi)
            np.testing.assert_allclose(a["xy"], b["xy"], rtol=1e-10, atol=1e-11, err_msg=what)
            np.testing.assert_allclose(a["c"], b["c"], rtol=1e-9, err_msg=what)
            np.testing.assert_allclose(a["u"], b["u"], rtol=1e-8, atol=1e-11, err_msg=what)
            nominal = b["u"]
            fast.set_nominal(nominal)
        fast.close()
        forced.close()

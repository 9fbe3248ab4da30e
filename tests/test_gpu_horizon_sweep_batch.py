"""GPU tests (-m gpu): every horizon H = 5 .. 26 through every rung of the batch rollout kernels (BatchForm, csrc/mppi_kernels.h:
Batch, Varied, Obst, Moving, Grid, each with and without the shifted weights), in the four-wave, the one-wave and the plain family,
each rung against the reference the rung's own suite uses.

The other batch suites run four residues of (H - 1) % 8 between them (0, 1, 3, 6: H = 9, 10, 15, 20); the masked PARTIAL producer
with a runtime step count has never run under a disc, moving-disc or grid term, and a time index that slips by one in a partial
block, or a wrong consumer width beside a term, would pass them.  tests/horizon_cases.py restates what each H selects,
tests/test_horizon_cases_cpu.py proves the coverage, tests/test_horizon_sweep_inputs_cpu.py pins the conditions on the inputs on
the oracle's rollouts (tests/horizon_sweep_inputs.py makes them: five instances, K = 130).

One handle per shift in {off, on} walks up the rungs with the same warm start, seeds and iteration at each; last_kernel() is
asserted at every rung:
  base, Varied   every instance against the oracle, with the shared and with its own parameters
                 (test_every_instance_matches_the_oracle_with_its_own_parameters: TOL_U, TOL_COST); NULL restores the base bits
  Obst           OC.discs_for, OC.check_penalty; an instance without discs or without weight keeps every bit
  Moving         OC.moving_discs_for, OC.check_moving (the static run of the same discs beside it); a velocity table of zeros
                 runs the MOVING kernels and gives the static bits
  Grid           on top of the moving discs: GC.check_identity, cost_on == fma(w, G, cost_off) in every bit.  Full body has no
                 one-wave GRID form (has_one_wave_form): in the one-wave family its grid rung reports the four-wave bits and the
                 identity is held within TOL_COST, as test_full_body_beyond_one_workgroup_per_cu_runs_the_four_wave_form
  shift on       every rung's costs bit-equal to shift off; u*, sum_w and n_zero_weight through UC.check_shift with E_SHIFT
  down           every rung's kernel and bits restored, as test_gpu_batch_forms.py
The one-wave family: the five instances repeated until the batch has more workgroups than the rule's threshold; the first five
are read back and checked.  The plain family: CCV_MPPI_KERNEL=v1.
"""
import numpy as np
import pytest

import batch_support as BS
import grid_cases as GC
import grid_reference as GR
import helpers
import horizon_cases as HC
import horizon_sweep_inputs as HI
import obstacle_cases as OC
import update_checks as UC
from batch_support import GRID, MOV, OV, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, capi

pytestmark = pytest.mark.gpu
B = HI.B
VARIED = capi.BATCH_KERNEL_VARIED
FAMILY = {"r4": capi.BATCH_KERNEL_FOUR_WAVE, "solo": capi.BATCH_KERNEL_ONE_WAVE, "plain": capi.BATCH_KERNEL_PLAIN}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def repetitions(model, family):
    """copies of the five instances: one, or (one-wave) as many as put the batch's workgroups past the rule's threshold"""
    if family != "solo":
        return 1
    per_instance = -(-HI.K // 64)
    threshold = (1 if model == "full_body" else 5) * BS.cus()
    return -(-(threshold + 1) // (per_instance * B))


def snapshot(bat, u, st):
    """the first five instances' read-backs (the form BS.snapshot gives, with the statistics beside their tuple)"""
    return [dict(u=u[b].copy(), st=BS.stats_tuple(st[b]), stats=st[b], c=bat.read_costs(b), w=bat.read_weights(b),
                 xy=bat.read_candidates(b)) for b in range(B)]


def walk(model, H, family, shift, plain_costs):
    """one handle up and down the rungs -> {rung: [B] costs} (shift off: what the shift-on walk is held against)"""
    c = HI.batch_case(model, H)
    p, reps = c.p, repetitions(model, family)
    fam = FAMILY[family]
    assert family == "plain" or BS.families(model, HI.K, B * reps)[1] == family
    x0, dt, xr, yr, yaw0, seeds, nom = [np.concatenate([a] * reps) for a in c.inputs]
    sh = SHIFT if shift else 0
    base_code = fam | ((SHIFT | VARIED) if shift else 0)
    what0 = "%s H=%d %s%s" % (model, H, family, " shift" if shift else "")
    bat = BatchController(p, B * reps, min_shift=shift)
    costs = {}

    def run(rung, code, params=None):
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, HI.IT)
        assert bat.last_kernel() == code, (what0, rung, hex(bat.last_kernel()), hex(code))
        snap = snapshot(bat, u, st)
        costs[rung] = [s["c"] for s in snap]
        if shift:
            for b in range(B):
                what = "%s %s b=%d" % (what0, rung, b)
                assert snap[b]["c"].tobytes() == plain_costs[rung][b].tobytes(), what   # costs: the shift-off run's bits
                q = params[b] if params else p
                UC.check_shift(what, snap[b]["c"], HI.oracle_iteration(model, H, params is not None)[b]["ctl"], q.lam, snap[b]["u"],
                               snap[b]["stats"].sum_w, snap[b]["w"], snap[b]["stats"], sens=False)
        return snap

    def against_oracle(rung, snap, varied):
        for b, ref in enumerate(HI.oracle_iteration(model, H, varied)):
            what = "%s %s b=%d" % (what0, rung, b)
            assert np.max(np.abs(snap[b]["c"] - ref["c"]) / ref["c"]) < BS.TOL_COST, what
            if not shift:   # (the oracle forms the reference's weights; the shifted update: check_shift, in run)
                assert helpers.rel_err(snap[b]["u"], ref["u"]) < BS.TOL_U, what

    def restored(rung, snap, want):
        assert all(BS.same_bits(want[b], snap[b]) for b in range(B)), (what0, "down to " + rung)

    # ---- base and Varied
    base = run("base", base_code)
    against_oracle("base", base, False)
    bat.set_params(c.seq * reps)
    var = run("varied", fam | VARIED | sh, params=c.seq)
    against_oracle("varied", var, True)
    assert any(var[b]["c"].tobytes() != base[b]["c"].tobytes() for b in range(B)), what0
    bat.set_params(None)
    restored("base", run("base", base_code), base)
    # ---- Obst
    bat.set_obstacles(c.discs * reps, np.tile(c.w_obs, reps))
    obst = run("obst", fam | OV | sh)
    for b in range(B):
        what = "%s obst b=%d n=%d" % (what0, b, len(c.discs[b]))
        OC.check_penalty(what, p, c.inputs[0][b], c.discs[b], c.w_obs[b], base[b], obst[b])
        if len(c.discs[b]) == 0 or c.w_obs[b] == 0.0:
            assert BS.same_bits(base[b], obst[b]), what
        else:
            assert not np.array_equal(base[b]["c"], obst[b]["c"]), what
    # ---- Moving: the same discs standing, under a table of zeros, moving
    bat.set_obstacles(c.mdiscs * reps, np.tile(c.w_obs, reps))
    sta = run("static", fam | OV | sh)
    bat.set_obstacle_velocities([np.zeros_like(v) for v in c.vels] * reps)
    zero = run("zero", fam | MOV | sh)
    bat.set_obstacle_velocities(c.vels * reps)
    mov = run("moving", fam | MOV | sh)
    for b in range(B):
        what = "%s moving b=%d n=%d" % (what0, b, len(c.mdiscs[b]))
        OC.check_moving(what, p, c.inputs[0][b], c.inputs[1][b], c.mdiscs[b], c.vels[b], c.w_obs[b], base[b], sta[b], mov[b])
        if len(c.mdiscs[b]) == 0 or c.w_obs[b] == 0.0:
            assert BS.same_bits(base[b], mov[b]), what
        else:
            assert not np.array_equal(sta[b]["c"], mov[b]["c"]), what
        assert BS.same_bits(sta[b], zero[b]), what
    # ---- Grid, on top of the moving discs
    one_wave_form = not (family == "solo" and model == "full_body")   # (has_one_wave_form, csrc/mppi_launch.h)
    grid_code = (fam if one_wave_form else capi.BATCH_KERNEL_FOUR_WAVE) | GRID | sh
    bat.set_grids([g.as_tuple() for g in c.maps], np.tile(c.map_of, reps), np.tile(c.w_grid, reps))
    grid = run("grid", grid_code)
    for b in range(B):
        what = "%s grid b=%d map=%d w=%g" % (what0, b, c.map_of[b], c.w_grid[b])
        if one_wave_form:
            if c.map_of[b] < 0:
                assert BS.same_bits(mov[b], grid[b]), what
                continue
            GC.check_identity(what, p, c.maps[c.map_of[b]], c.w_grid[b], mov[b], grid[b])
            if c.w_grid[b] == 0.0:
                assert BS.same_bits(mov[b], grid[b]), what
            else:
                assert not np.array_equal(mov[b]["c"], grid[b]["c"]), what
        elif c.map_of[b] < 0 or c.w_grid[b] == 0.0:   # (the term-off run is another kernel's: no term, the same costs within TOL_COST)
            assert np.max(np.abs(grid[b]["c"] - mov[b]["c"]) / np.abs(mov[b]["c"])) < BS.TOL_COST, what
            assert helpers.rel_err(grid[b]["u"], mov[b]["u"]) < BS.TOL_U, what
        else:   # (the identity within TOL_COST, G from the term-on states)
            g = c.maps[c.map_of[b]]
            P = grid[b]["xy"][:, :GR.n_covered(model, H)]
            share_in, share_out, cells = GR.coverage(g, P)
            assert share_in >= 0.25 and share_out >= 0.05 and cells >= 50, (what, share_in, share_out, cells)
            want = GR.cost_on(mov[b]["c"], c.w_grid[b], GR.grid_sum(g, P))
            assert np.max(np.abs(grid[b]["c"] - want) / np.abs(want)) < BS.TOL_COST, what
    # ---- down
    bat.set_grids(None)
    restored("moving", run("moving", fam | MOV | sh), mov)
    bat.set_obstacle_velocities(None)
    restored("static", run("static", fam | OV | sh), sta)
    bat.set_obstacles(None)
    restored("base", run("base", base_code), base)
    bat.close()
    return costs


@pytest.mark.parametrize("family", ["r4", "solo", "plain"])
@pytest.mark.parametrize("H", HC.BATCH_H)
@pytest.mark.parametrize("model", HC.MODELS)
def test_every_rung_matches_its_reference(monkeypatch, model, H, family):
    if family == "plain":
        monkeypatch.setenv("CCV_MPPI_KERNEL", "v1")
    else:
        monkeypatch.delenv("CCV_MPPI_KERNEL", raising=False)
    print("[horizon sweep batch] %s H=%d %s: (nblocks, nctl_last, nv_last, tail, nfull, prune) = %s" % (model, H, family, HC.block_shape(model, H)))
    plain_costs = walk(model, H, family, False, None)
    walk(model, H, family, True, plain_costs)


def test_one_wave_batch_with_an_instance_on_the_reference_clamp():
    """An instance whose bounds are out of order in one dimension gets the reference's compare-and-select clamp
    (fill_params: fast_clamp off for that instance).  In a batch large enough for the one-wave kernel -- where
    test_clamp_form_is_chosen_per_instance, sixteen workgroups per instance and four instances, never gets -- that
    instance's workgroups must still stage their warm start: every one of the first five instances against the oracle with
    its own parameters, H = 13 (four control steps in the last block: the PARTIAL producer in both clamp forms)."""
    model, H = "diff_drive", 13
    c = HI.batch_case(model, H)
    reps = repetitions(model, "solo")
    seq = list(c.seq)
    seq[1] = seq[1].with_(u_min=(0.6, -2.0), u_max=(0.2, 2.0))   # v: u_min > u_max
    x0, dt, xr, yr, yaw0, seeds, nom = [np.concatenate([a] * reps) for a in c.inputs]
    bat = BatchController(seq * reps, B * reps)
    bat.set_nominal(nom)
    u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, HI.IT)
    assert bat.last_kernel() == capi.BATCH_KERNEL_ONE_WAVE | VARIED
    for b in range(B):
        o = helpers.oracle_for(seq[b])
        o.set_nominal(nom[b])
        u_o = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=HI.IT)
        assert np.max(np.abs(bat.read_costs(b) - o.costs()) / o.costs()) < BS.TOL_COST, b
        assert helpers.rel_err(u[b], u_o) < BS.TOL_U, b
    bat.close()

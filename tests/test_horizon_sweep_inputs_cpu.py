"""The conditions on the inputs of the batch horizon sweep, on the reference alone (no GPU): at every model and horizon of the
sweep, at its K = 130, the oracle's rollouts give every instance with discs a non-zero reference penalty on 10 % .. 90 % of the
samples -- static (OC.discs_for, obstacle_reference) and moving (OC.moving_discs_for, moving_obstacle_reference) -- and every
instance with a map (GR.map_over) at least 25 % of its covered states in bounds, at least 5 % out of bounds and at least 50
distinct cells hit.  The GPU tests assert the same on the device's own states; this one says the inputs were not tuned on them."""
import numpy as np
import pytest

import grid_reference as GR
import horizon_cases as HC
import horizon_sweep_inputs as HI
import moving_obstacle_reference as MR
import obstacle_reference as OR


@pytest.mark.parametrize("model", HC.MODELS)
def test_discs_and_maps_meet_their_conditions_at_every_horizon(model):
    worst = dict(lo=1.0, hi=0.0, share_in=1.0, share_out=1.0, cells=10**9)
    for H in HC.BATCH_H:
        c = HI.batch_case(model, H)
        x0, dt = c.inputs[0], c.inputs[1]
        for b in range(HI.B):
            P = c.states[b]
            what = (model, H, b)
            assert P.shape == (HI.K, HC.nstates(model, H), 2)
            if len(c.discs[b]):
                tot, _ = OR.sample_penalty(P, x0[b, :2], c.discs[b], HI.OC.W_OBS)
                mtot, _ = MR.sample_penalty(P, x0[b, :2], np.arange(P.shape[1]), dt[b], c.mdiscs[b], c.vels[b], HI.OC.W_OBS)
                for frac in (float(np.mean(tot > 0)), float(np.mean(mtot > 0))):
                    assert 0.10 <= frac <= 0.90, (what, frac)
                    worst["lo"], worst["hi"] = min(worst["lo"], frac), max(worst["hi"], frac)
            if c.map_of[b] >= 0:
                g = c.maps[c.map_of[b]]
                share_in, share_out, cells = GR.coverage(g, P)
                assert share_in >= 0.25 and share_out >= 0.05 and cells >= 50, (what, share_in, share_out, cells)
                assert g.nx != g.ny and g.nx & (g.nx - 1) and g.ny & (g.ny - 1)
                assert len(np.unique(g.cells)) == g.cells.size and not np.any(g.cells == g.outside)
                worst["share_in"], worst["share_out"] = min(worst["share_in"], share_in), min(worst["share_out"], share_out)
                worst["cells"] = min(worst["cells"], cells)
    print("[horizon sweep inputs] %s: disc shares %.2f .. %.2f; maps: in >= %.2f, out >= %.2f, cells >= %d"
          % (model, worst["lo"], worst["hi"], worst["share_in"], worst["share_out"], worst["cells"]))


def test_the_salted_case_is_the_one_that_needs_it():
    """steering H = 5 with the default salt: a moving-disc instance every sample of which is penalised (horizon_cases.BATCH_SALT)"""
    assert HC.BATCH_SALT == {("steering_diff_drive", 5): HC.batch_salt("steering_diff_drive", 5)}
    p = HI.BS.MODEL_DEFAULTS["steering_diff_drive"](HI.K, 5)
    inputs = HI.BS.instance_inputs(p, HI.B)
    x0, dt, _, _, _, seeds, nom = inputs
    mdiscs, vels = HI.OC.moving_discs_for(p, inputs, it=HI.IT)
    fracs = []
    for b in range(HI.B):
        if len(mdiscs[b]):
            P = HI.OC.oracle_states(p, x0[b], dt[b], nom[b], seeds[b], HI.IT)
            tot, _ = MR.sample_penalty(P, x0[b, :2], np.arange(P.shape[1]), dt[b], mdiscs[b], vels[b], HI.OC.W_OBS)
            fracs.append(float(np.mean(tot > 0)))
    assert max(fracs) > 0.90, fracs

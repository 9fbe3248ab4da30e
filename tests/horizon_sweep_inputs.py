"""Inputs of the batch horizon sweep (tests/test_gpu_horizon_sweep_batch.py), made on the CPU from the oracle's rollouts and
shared by its three kernel families: five instances of BS.instance_inputs, the static discs of OC.discs_for, the moving discs of
OC.moving_discs_for, one occupancy map per instance from GR.map_over.  tests/test_horizon_sweep_inputs_cpu.py pins the conditions
that keep the sweep from passing vacuously, on the reference alone; no GPU is needed here.

Instances, in order (the roles of the disc and grid suites): discs 0 / 1 / 3 / 4 / 32 (OC.NS), instance 3's disc weight 0;
no map / map / map / map with weight 0 / map with another weight (grid_cases.W_GRID), every map its instance's own."""
import functools

import numpy as np

import batch_support as BS
import grid_reference as GR
import helpers
import horizon_cases as HC
import obstacle_cases as OC

B = 5
K = 130          # three workgroups per instance, two live lanes in the last
IT = 0           # the iteration of every rung
W_GRID = (0.0, 0.01, 0.01, 0.0, 0.025)   # (grid_cases.W_GRID)
MAP_OF = (-1, 0, 1, 2, 3)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def batch_case(model, H, K=K):
    c = Case()
    c.p = BS.MODEL_DEFAULTS[model](K, H)
    c.inputs = BS.instance_inputs(c.p, B, salt=HC.batch_salt(model, H))
    x0, dt, xr, yr, yaw0, seeds, nom = c.inputs
    c.discs = OC.discs_for(c.p, c.inputs, it=IT)
    c.mdiscs, c.vels = OC.moving_discs_for(c.p, c.inputs, it=IT)
    c.w_obs = np.full(B, OC.W_OBS)
    c.w_obs[3] = 0.0   # discs, but no weight
    # (oracle_states: already cut to the states the path term covers)
    c.states = [OC.oracle_states(c.p, x0[b], dt[b], nom[b], seeds[b], IT) for b in range(B)]
    c.map_of = np.array(MAP_OF, dtype=np.int32)
    c.w_grid = np.array(W_GRID)
    c.maps = [GR.map_over(c.states[b], salt=b) for b in range(B) if MAP_OF[b] >= 0]
    c.seq = BS.varied(c.p, B)
    return c


@functools.lru_cache(maxsize=None)
def oracle_iteration(model, H, varied, K=K):
    """[B] dicts (u, c, ctl): the oracle's iteration IT of every instance, with the shared parameters or with c.seq's"""
    c = batch_case(model, H, K)
    x0, dt, xr, yr, yaw0, seeds, nom = c.inputs
    out = []
    for b in range(B):
        o = helpers.oracle_for(c.seq[b] if varied else c.p)
        o.set_nominal(nom[b])
        u = o.iterate(x0[b], dt[b], xr[b], yr[b], yaw0[b], seed=int(seeds[b]), rng="philox", iteration=IT)
        out.append(dict(u=np.array(u), c=np.array(o.costs()), ctl=np.array(o.get_controls())))
    return out

"""Cases, inputs and the checker of the occupancy-grid term.

Instances of a batch of five, in order: no map; map 0; map 1; map 0 with weight 0; map 1 with another weight.  Instances 3 and 4
stand near instances 1 and 2 (grid_inputs), whose poses place the maps (grid_reference.map_ahead).  check_identity holds cost_on
against fma(w_grid, G_ref, cost_off) bit for bit, with G_ref from tests/grid_reference.py on the states the device stored, and
asserts the conditions on the inputs.

tests/test_gpu_batch_grid.py exercises the checker on every case, the batch horizon sweep borrows it;
tests/test_grid_reference.py checks the same conditions on the oracle's rollouts, without a GPU.  Needs no GPU to import.
"""
import numpy as np

import batch_support as BS
import grid_reference as GR
import obstacle_cases as OC

W_GRID = (0.0, 0.01, 0.01, 0.0, 0.025)   # (not dyadic: the products round)
MAP_OF = (-1, 0, 1, 0, 1)
CASES = OC.CASES
PLAIN_CASE = ("diff_drive", 1000, 15, 5, {}, "plain")


def roles(B):
    """(map_of [B], weight [B]): the five roles dealt round; a batch of two: a map and none"""
    if B == 2:
        return np.array([0, -1], dtype=np.int32), np.array([W_GRID[1], 0.0])
    return np.array([MAP_OF[b % 5] for b in range(B)], dtype=np.int32), np.array([W_GRID[b % 5] for b in range(B)])


def grid_inputs(p, B, salt=0):
    """BS.instance_inputs with instances 3 and 4 of every five moved beside instances 1 and 2 (pose, dt and window theirs, a
    little to the side and turned; seeds and warm starts their own), so that one map serves both"""
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B, salt)
    for b in range(B):
        if b % 5 in (3, 4) and B >= 5:
            a = b - 2
            x0[b], dt[b], xr[b], yr[b], yaw0[b] = x0[a], dt[a], xr[a], yr[a], yaw0[a]
            x0[b, 1] += 0.03
            x0[b, 2] += 0.05
    return x0, dt, xr, yr, yaw0, seeds, nom


def maps_for(p, inputs):
    """(two maps, map_of, weight): map m placed from the pose of the first instance that uses it, on the side its warm start
    drives to (the full-body warm starts of instance_inputs, drawn around the middle of the speed bounds, reverse)"""
    x0, dt, nom = inputs[0], inputs[1], inputs[6]
    map_of, w = roles(len(dt))
    maps = []
    for m in (0, 1):
        b = int(np.argmax(map_of == m)) if np.any(map_of == m) else 0
        maps.append(GR.map_ahead(x0[b, :3], p.v_ref, dt[b], p.horizon, salt=m, backwards=bool(np.mean(nom[b, :, 0]) < 0.0)))
    return maps, map_of, w


def check_identity(what, p, g, w, off, on, conditions=True):
    """states bit-equal; cost_on == fma(w, G_ref, cost_off) in every bit; the conditions on the inputs"""
    assert on["xy"].tobytes() == off["xy"].tobytes(), what
    P = on["xy"][:, :GR.n_covered(p.model, p.horizon)]
    share_in, share_out, cells = GR.coverage(g, P)
    G = GR.grid_sum(g, P)
    want = GR.cost_on(off["c"], w, G)
    bad = int(np.sum(want.view(np.uint64) != on["c"].view(np.uint64)))
    print("[grid] %s: in %.2f out %.2f cells %d, G %.6g .. %.6g, costs that differ %d of %d" % (what, share_in, share_out, cells, G.min(), G.max(), bad, len(G)))
    if conditions:
        assert share_in >= 0.25 and share_out >= 0.05 and cells >= 50, (what, share_in, share_out, cells)
    assert bad == 0, (what, bad)

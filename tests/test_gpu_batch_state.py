"""GPU test (-m gpu): what a batch handle computes depends on the state its setters left, not on the road by which it got there.

Two handles reach the same final state -- per-instance parameters, shifted weights, static discs with velocities (0, 1 and 3
discs over the three instances), two maps (used as map 0, none, map 1) and, in the first case, the fleet term with prediction
-- by two roads.  Road A applies the setters once each in the order of the kernels' forms (BatchForm, csrc/mppi_kernels.h).
Road B applies them in roughly the reverse order with detours: every term switched on, off and on again, the discs set twice
(which drops their velocities), the maps first and, off and on once more, last.  Every device table the kernels read (the
parameter table, the disc and velocity tables, the fleet's static counts: sync_tables, csrc/capi_batch_config.hip) then has to
hold the same values, and everything a tick leaves is compared bit for bit.

Diff drive K = 128 and full body K = 64 at H = 15, B = 3: the four-wave family with six control steps in the horizon's last
block (the TAIL form), the smallest shapes at which every table is read.  The fleet term's discs share the static discs'
weight (the fleet's setter replaces it), so that the final state does not depend on which of the two came last.
"""
import numpy as np
import pytest

import batch_support as BS
import fleet_support as FS
import fleet_velocity_reference as FV
from ccv_mppi_path_tracker_amd import BatchController, capi

pytestmark = pytest.mark.gpu
B, H, TICKS = 3, 15, 6
W_OBS = 50.0
FLEET = (np.array([0.15, 0.2, 0.25]), 1.5, 2, W_OBS)   # radius, range, max_neighbours, weight
WANT_BITS = (capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_VARIED | capi.BATCH_KERNEL_SHIFT | capi.BATCH_KERNEL_OBST |
             capi.BATCH_KERNEL_MOVING | capi.BATCH_KERNEL_GRID)
SHAPES = [("diff_drive", 128), ("full_body", 64)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def terms(p, at):
    """the final state's additions around the instances' positions at [B][>= 2]: (parameters, discs, velocities, maps' arguments)"""
    discs = [np.zeros((0, 3)), np.array([[at[1, 0] + 0.3, at[1, 1] + 0.1, 0.3]]),
             np.concatenate([[[at[2, 0], at[2, 1] - 0.3, 0.25]], FS.far_discs(2)])]
    velocities = [np.zeros((0, 2)), np.array([[-0.1, 0.05]]), np.array([[0.08, 0.12], [0.3, -0.2], [-0.4, 0.6]])]
    cells = (0.25 + np.random.default_rng(7).random((24, 24))).astype(np.float32)
    maps = ([(cells, (at[0, 0] - 3.0, at[0, 1] - 3.0), 0.25, 0.5), (cells.T.copy(), (at[2, 0] - 3.0, at[2, 1] - 3.0), 0.25, 0.0)],
            [0, -1, 1], [0.01, 0.0, 0.025])
    return BS.varied(p, B), discs, velocities, maps


def road_a(bat, seq, discs, velocities, maps, fleet):
    bat.set_params(seq)
    bat.set_min_shift(True)
    bat.set_obstacles(discs, W_OBS)
    bat.set_obstacle_velocities(velocities)
    bat.set_grids(*maps)
    if fleet:
        bat.resident_set_fleet(*FLEET)
        bat.resident_set_fleet_prediction(True)


def road_b(bat, seq, discs, velocities, maps, fleet):
    bat.set_grids(*maps)
    if fleet:
        bat.resident_set_fleet(*FLEET)
        for on in (True, False, True):
            bat.resident_set_fleet_prediction(on)
    bat.set_obstacles(discs, W_OBS)
    bat.set_obstacle_velocities(velocities)
    bat.set_obstacles(discs, W_OBS)   # (drops the velocities)
    assert not any(v.any() for v in bat.get_obstacle_velocities())
    bat.set_obstacle_velocities(velocities)
    for on in (True, False, True):
        bat.set_min_shift(on)
    for s in (seq, None, seq):
        bat.set_params(s)
    bat.set_grids(None)
    bat.set_grids(*maps)


@pytest.mark.parametrize("model,K", SHAPES, ids=["dd", "fb"])
def test_two_roads_to_one_state_with_the_fleet_term(model, K):
    """6 resident ticks from the same poses and warm start: u*, poses, indices, windows and costs (FS.bits), the _read_fleet
    counts and rows, the _read_fleet_velocities rows and last_kernel() are equal after every tick."""
    p = FS.params(model, K, H)
    assert BS.families(model, K, B)[1] == "r4"
    s0, seeds, paths = FS.fleet_start(p, B)
    seq, discs, velocities, maps = terms(p, s0)
    nom = np.zeros((B, H - 1, p.udim))
    n_static = np.array([len(d) for d in discs])
    sv = FV.table(velocities)
    out = []
    for road in (road_a, road_b):
        bat = FS.make(p, B, False, None, 0.0, paths, s0, seeds)
        road(bat, seq, discs, velocities, maps, True)
        bat.resident_set_poses(s0, seeds)
        bat.set_nominal(nom)
        ticks = []
        for it in range(TICKS):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            ns, nt, xyr = bat.resident_read_fleet()
            ticks.append((FS.bits(bat), ns.tolist(), nt.tolist(), xyr.tobytes(), bat.resident_read_fleet_velocities(), bat.last_kernel()))
        bat.close()
        out.append(ticks)
    a, b = out
    # the conditions under which the comparison means something: every table is read, and the fleet's rows are not empty
    assert all(t[5] == WANT_BITS for t in a), hex(a[0][5])
    assert all(t[1] == n_static.tolist() for t in a)
    assert any((np.array(t[2]) > n_static).any() for t in a)                       # a neighbour's disc
    assert any((t[4] != sv).any() for t in a)                                      # ... with a velocity that is not zero
    assert all((t[4][y, :n] == sv[y, :n]).all() for t in a for y, n in enumerate(n_static))   # beside the static rows
    for it, (ta, tb) in enumerate(zip(a, b)):
        for key in ta[0]:
            assert ta[0][key] == tb[0][key], (key, it)
        assert ta[1:4] == tb[1:4], it
        assert ta[4].tobytes() == tb[4].tobytes(), it
        assert ta[5] == tb[5], it


@pytest.mark.parametrize("model,K", SHAPES, ids=["dd", "fb"])
def test_two_roads_to_one_state_without_the_fleet_term(model, K):
    """one iterate from the same inputs: u* and every instance's costs are equal"""
    p = BS.MODEL_DEFAULTS[model](K, H)
    assert BS.families(model, K, B)[1] == "r4"
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    seq, discs, velocities, maps = terms(p, x0)
    out = []
    for road in (road_a, road_b):
        bat = BatchController(p, B)
        road(bat, seq, discs, velocities, maps, False)
        bat.set_nominal(nom)
        u, _ = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 3)
        out.append((bat.last_kernel(), u.tobytes(), [bat.read_costs(i).tobytes() for i in range(B)]))
        bat.close()
    assert out[0][0] == WANT_BITS, hex(out[0][0])
    assert out[0] == out[1]

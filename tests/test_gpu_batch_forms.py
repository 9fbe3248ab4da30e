"""GPU test (-m gpu) of one batch handle walked up and down the ladder of its kernels' forms (BatchForm, csrc/mppi_kernels.h):
plain batch -> set_params -> set_min_shift -> set_obstacles -> velocities -> set_grids, then every step undone in reverse order.
Every rung launches from another translation unit (k_batch.hip / k_r4.hip, k_batch_shift.hip, k_batch_obst_shift.hip,
k_batch_moving_shift.hip, k_batch_grid_shift.hip, and k_batch_varied.hip on the way), so one process runs the switch from a
launch's plan to its unit across all of them.  At every rung the same warm start, seeds and iteration: last_kernel() is the
rung's bits, and on the way down u* and every instance's costs are bit-equal to what the same rung gave on the way up.

The four-wave family only (its two instantiations by the horizon's last block: H = 9 has no control step there, H = 15 has six,
the TAIL form); the one-wave family needs more than five blocks per CU and is walked by the grid and moving suites.
"""
import numpy as np
import pytest

import batch_support as BS
from ccv_mppi_path_tracker_amd import BatchController, capi

pytestmark = pytest.mark.gpu
VARIED, SHIFT = capi.BATCH_KERNEL_VARIED, capi.BATCH_KERNEL_SHIFT
OBST, MOVING, GRID = capi.BATCH_KERNEL_OBST, capi.BATCH_KERNEL_MOVING, capi.BATCH_KERNEL_GRID
B = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.mark.parametrize("model,K,H", [("diff_drive", 128, 9), ("diff_drive", 128, 15), ("full_body", 64, 15)])
def test_up_and_down_the_ladder(model, K, H):
    p = BS.MODEL_DEFAULTS[model](K, H)
    assert BS.families(model, K, B)[1] == "r4"
    x0, dt, xr, yr, yaw0, seeds, nom = BS.instance_inputs(p, B)
    # discs over the start (whichever way the warm start drives, the first states lie inside; instance 1: a second one beside it),
    # moving away from it; a map of positive cells around the start
    discs = [np.array([[x0[0, 0], x0[0, 1], 0.3]]), np.array([[x0[1, 0], x0[1, 1], 0.25], [x0[1, 0] + 0.2, x0[1, 1], 0.2]])]
    velocities = [np.array([[0.1, -0.05]]), np.array([[-0.08, 0.06], [0.0, 0.1]])]
    cells = (0.25 + np.random.default_rng(7).random((24, 24))).astype(np.float32)
    maps = [(cells, (x0[0, 0] - 3.0, x0[0, 1] - 3.0), 0.25, 0.5), (cells.T.copy(), (x0[1, 0] - 3.0, x0[1, 1] - 3.0), 0.25, 0.0)]

    bat = BatchController(p, B)

    def run():
        bat.set_nominal(nom)
        u, _ = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 3)
        return bat.last_kernel(), u.copy(), [bat.read_costs(b) for b in range(B)]

    # (what the rung adds to the bits of the one below, its setter, the setter that undoes it, whether it changes the costs)
    rungs = [(VARIED, lambda: bat.set_params(BS.varied(p, B)), lambda: bat.set_params(None), True),
             (SHIFT, lambda: bat.set_min_shift(True), lambda: bat.set_min_shift(False), False),
             (OBST, lambda: bat.set_obstacles(discs, 5.0), lambda: bat.set_obstacles(None), True),
             (MOVING, lambda: bat.set_obstacle_velocities(velocities), lambda: bat.set_obstacle_velocities(None), True),
             (GRID, lambda: bat.set_grids(maps, [0, 1], [0.01, 0.025]), lambda: bat.set_grids(None), True)]
    bits = capi.BATCH_KERNEL_FOUR_WAVE
    up = [(bits,) + run()[1:]]
    assert bat.last_kernel() == bits
    for add, do, _, changes_costs in rungs:
        do()
        bits |= add
        kernel, u, costs = run()
        print("[forms] %s K=%d H=%d up: kernel %#x" % (model, K, H, kernel))
        assert kernel == bits
        if changes_costs:   # (the rung's term is in the costs: the setter reached the kernel)
            assert any(costs[b].tobytes() != up[-1][2][b].tobytes() for b in range(B)), hex(bits)
        up.append((bits, u, costs))
    for i in range(len(rungs) - 1, -1, -1):
        rungs[i][2]()
        want_bits, want_u, want_costs = up[i]
        kernel, u, costs = run()
        print("[forms] %s K=%d H=%d down: kernel %#x" % (model, K, H, kernel))
        assert kernel == want_bits
        assert u.tobytes() == want_u.tobytes(), hex(want_bits)
        assert all(costs[b].tobytes() == want_costs[b].tobytes() for b in range(B)), hex(want_bits)
    bat.close()

"""What the tests of the device-inflated costmaps share (DESIGN.md sections 10k to 10n: set_occupancy and its patches, rolls
and scans): the arguments of one occupancy map, the derived cells of a handle, bit equality of arrays, the inflation profile
and the occupancy layers of the twin tests, everything a tick leaves as bytes, the cells a rollout reads, the process's
resident memory, and the door's block as a marking and a clearing scan.

Used by tests/test_gpu_batch_costmap.py, tests/test_gpu_batch_roll.py and tests/test_gpu_batch_scan.py, which hold the derived
cells against tests/costmap_reference.py bit for bit; tests/test_scan_reference.py pins block_scans on the CPU restatement of
the door (tools/costmap_door_cpu.py).  Needs no GPU to import.
"""
import os
import sys

import numpy as np

import costmap_reference as CR
import grid_reference as GR
import scan_reference as SR
from ccv_mppi_path_tracker_amd import batch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import costmap_door_cpu as CD  # noqa: E402

INFLATION = batch.inflation_profile(0.2, 0.05, kind="exponential", lethal=3.0, inscribed=2.0, inscribed_m=0.05, scaling=8.0, free_value=0.125)
CLEAR_TICK = 20   # the clearing scan is enqueued right after this tick's step


def occ_map(cells, threshold=128, origin=(0.0, 0.0), resolution=0.05, outside=CR.OUTSIDE):
    return (cells, origin, resolution, outside, threshold)


def derived(bat, m=0):
    return bat.get_grids()[0][m][0]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def layer_like(g, seed):
    """an occupancy layer with the geometry of a grid_reference map: 6 % of the cells occupied"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((g.ny, g.nx)) < 0.06, 255, 0).astype(np.uint8)


def tick_bits(bat):
    B = bat.B
    return [bat.get_nominal().tobytes()] + [bat.read_costs(b).tobytes() + bat.read_weights(b).tobytes() + bat.read_candidates(b).tobytes()
                                            for b in range(B)]


def cells_hit(geo, P):
    """the flat cell indices the covered states P [K][n][2] read"""
    _, inside, idx = GR.lookup(geo, P[..., 0], P[..., 1])
    return np.unique(idx[inside])


def _rss_kb():
    for line in open("/proc/self/status"):
        if line.startswith("VmRSS:"):
            return int(line.split()[1])
    return 0


def block_scans():
    """(sensor cell, the marking scan, the clearing scan) of the door's block (tools/costmap_door_cpu.py), seen from the start cell:
    a hit on every cell of the block; then a miss through every cell of the block -- the ray to 2 c - s passes through c exactly,
    (2 a_c 2 b_c + 2 a_c) div (4 a_c) = b_c.  The marked layer is the door's patched one, so its CPU restatement applies as it is;
    the cleared one is the empty layer again."""
    x0, y0, patch = CD.block_patch()
    s = (int(np.floor((CD.START[0] - CD.ORIGIN[0]) / CD.RESOLUTION)), int(np.floor((CD.START[1] - CD.ORIGIN[1]) / CD.RESOLUTION)))
    block = np.array([(x, y) for y in range(y0, y0 + patch.shape[0]) for x in range(x0, x0 + patch.shape[1])], dtype=np.int64)
    through = 2 * block - np.array(s, dtype=np.int64)
    marked = SR.apply_scan(CD.empty_layer(), s, block, np.ones(len(block), dtype=np.uint8))
    want = CR.apply_patch(CD.empty_layer(), x0, y0, patch)
    assert same(marked, want), ("block_scans: the marking scan is not the door's patch", marked.shape, want.shape,
                                int(np.count_nonzero(marked)), int(np.count_nonzero(want)))
    cleared = SR.apply_scan(marked, s, through, np.zeros(len(block), dtype=np.uint8))
    assert same(cleared, CD.empty_layer()), ("block_scans: the clearing scan leaves cells", cleared.shape,
                                             int(np.count_nonzero(cleared)), int(np.count_nonzero(CD.empty_layer())))
    return s, (block, np.ones(len(block), dtype=np.uint8)), (through, np.zeros(len(block), dtype=np.uint8))

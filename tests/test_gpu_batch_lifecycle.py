"""GPU tests (-m gpu) of what a batch handle owns on the device: every part that allocates is switched on, used and let go, and the
device's free memory is read before and after (torch.cuda.mem_get_info), with the bound the other create/destroy tests use.

The sizes make every part that holds a large array allocate at least 1 MiB per cycle (B = 8, K = 64, H = 15: the maps' layers and
cells, the world, the sensing read-back of capi.SENSE_MAX_BEAMS beams, the kept plan fields, the traces), so that one array left
behind in 30 cycles is 30 MiB against the 8 MiB bound.  The small [B] tables are below what a memory reading sees: that no owner was
missed there is tests/test_owned_resources.py's to check.
"""
import numpy as np
import pytest

import batch_support as BS
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIError
from costmap_support import same

pytestmark = pytest.mark.gpu
B, K, H = 8, 64, 15
RES = 0.25
CYCLES, WARMUP, BOUND = 30, 3, 8 * 2**20
MAP_OF = np.array([0, 0, 0, 0, 1, -1, -1, -1], dtype=np.int32)
SIZES = ((512, 512), (200, 200))       # (nx, ny) of the two maps; the second satisfies 202 * 202 <= capi.PLAN_MAX_FIELD
WORLD = (1024, 1024)
INFLATION = batch.inflation_profile(1.0, RES)
CAPACITY = 1024


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def layer(nx, ny, seed):
    """an occupancy layer, 2 % of the cells occupied, none near the robots' row of cells"""
    cells = np.where(np.random.default_rng(seed).random((ny, nx)) < 0.02, 255, 0).astype(np.uint8)
    cells[:40] = 0
    return cells


LAYERS = [layer(nx, ny, 7 + m) for m, (nx, ny) in enumerate(SIZES)]
WORLD_CELLS = layer(WORLD[0], WORLD[1], 3)
FLOAT_MAPS = [np.random.default_rng(11 + m).random((ny, nx)).astype(np.float32) for m, (nx, ny) in enumerate(SIZES)]
ANCHORS = np.zeros((2, 2), dtype=np.int32)


def line_paths(n):
    """B straight paths of n poses one cell apart, all inside both maps"""
    return [(2.0 + RES * np.arange(n, dtype=np.float64), np.full(n, 2.0 + 0.5 * b)) for b in range(B)]


def occupancy_maps():
    return [(l, (0.0, 0.0), RES, 0.0, 128) for l in LAYERS]


def set_poses(bat, paths):
    st = np.zeros((B, 3))
    for b, (px, py) in enumerate(paths):
        st[b, 0], st[b, 1] = px[0], py[0]
    bat.resident_set_poses(st, np.array([BS.instance_seed(b) for b in range(B)], dtype=np.uint64))


def memory_shrinks_by(cycle):
    import torch
    for _ in range(WARMUP):   # runtime pools settle
        cycle()
    torch.cuda.synchronize()
    free0, _total = torch.cuda.mem_get_info()
    for _ in range(CYCLES):
        cycle()
    torch.cuda.synchronize()
    free1, _total = torch.cuda.mem_get_info()
    print("free0 - free1 = %d bytes (%.2f MiB) over %d cycles" % (free0 - free1, (free0 - free1) / 2**20, CYCLES))
    return free0 - free1


def test_batch_with_everything_set_create_destroy_returns_all_device_memory():
    p = configs.diff_drive_defaults(K, H)
    params = BS.varied(p, B)
    paths = line_paths(120)
    discs = [np.array([[30.0 + b, 40.0, 0.5], [35.0, 45.0 + b, 0.25]]) for b in range(B)]
    velocities = [np.array([[0.1, 0.0], [0.0, -0.1]])] * B
    beams = batch.beam_fan(capi.SENSE_MAX_BEAMS, 40)

    def cycle():
        bat = BatchController(params, B, num_samples=K, min_shift=True)
        bat.set_obstacles(discs, 1.0, velocities)
        bat.set_occupancy(occupancy_maps(), INFLATION, MAP_OF, 1.0)
        bat.set_world(WORLD_CELLS, 128, (0.0, 0.0), RES, ANCHORS, capi.SENSE_MAX_BEAMS)
        bat.resident_set_paths(paths, RES)
        set_poses(bat, paths)
        bat.resident_set_fleet(0.3, 5.0, 3, 1.0)
        bat.resident_set_fleet_prediction(True)
        bat.resident_set_plan(CAPACITY, keep_fields=True)
        bat.roll_occupancy([0], 1, 0)   # (the handle's first roll: the second set of layers and cells)
        bat.update_occupancy(0, 100, 100, np.full((8, 8), 255, dtype=np.uint8))
        bat.scan_occupancy([1], [(20, 20)], [np.array([[60, 20], [20, 70], [5, 5]], dtype=np.int32)], [np.array([1, 0, 1], dtype=np.uint8)])
        bat.update_world(300, 300, np.full((4, 4), 255, dtype=np.uint8))
        bat.resident_sense([4], beams)
        bat.resident_plan([4], [(150, 150)], 0.5)
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        bat.resident_step_enqueue(p.dt, 1)
        bat.close()   # (with the second tick's update still pending and the ring's events unwaited)

    lost = memory_shrinks_by(cycle)
    assert lost < BOUND, "device memory shrank by %.1f MiB over %d create/destroy cycles" % (lost / 2**20, CYCLES)


def test_one_batch_whose_parts_are_replaced_keeps_no_device_memory():
    p = configs.diff_drive_defaults(K, H)
    bat = BatchController(p, B, num_samples=K)
    short, long_ = line_paths(60), line_paths(120)
    float_maps = [(c, (0.0, 0.0), RES, 0.0) for c in FLOAT_MAPS]

    def state_error(call):
        with pytest.raises(MPPIError) as err:
            call()
        return err.value.code == capi.ERR_STATE

    def cycle():
        bat.set_occupancy(occupancy_maps(), INFLATION, MAP_OF, 1.0)
        geo = bat.get_occupancy()
        assert [(g[3], g[4]) for g in geo] == list(SIZES) and geo[0][0] == (0.0, 0.0)
        assert state_error(bat.get_world)
        bat.roll_occupancy([0], 1, 0)
        assert bat.get_occupancy()[0][0] == (RES, 0.0) and bat.get_occupancy()[1][0] == (0.0, 0.0)
        bat.set_world(WORLD_CELLS, 128, (0.0, 0.0), RES, ANCHORS, capi.SENSE_MAX_BEAMS)
        bat.set_world(WORLD_CELLS[:, :1000], 127, (0.0, 0.0), RES, ANCHORS, 64)
        origin, res, nx, ny, thr, anchors, max_beams = bat.get_world()
        assert (origin, res, nx, ny, thr, max_beams) == ((0.0, 0.0), RES, 1000, WORLD[1], 127, 64) and same(anchors, ANCHORS)
        bat.set_grids(float_maps, MAP_OF, 2.0)   # (drops layers and world)
        assert bat.get_occupancy() == [] and state_error(bat.get_world)
        maps, map_of, weight = bat.get_grids()
        assert len(maps) == 2 and all(same(m[0], c) for m, c in zip(maps, FLOAT_MAPS))
        assert same(map_of, MAP_OF) and same(weight, np.full(B, 2.0))
        bat.set_grids(None)
        maps, map_of, weight = bat.get_grids()
        assert maps == [] and (map_of == -1).all() and (weight == 0.0).all()
        bat.resident_set_paths(long_, RES)   # (twice as long: a new array)
        bat.resident_set_plan(CAPACITY, keep_fields=True)
        cap, keep = bat.resident_get_plan()
        assert (cap == CAPACITY).all() and keep
        x, y = bat.resident_read_path(3)
        assert same(x, long_[3][0]) and same(y, long_[3][1])
        bat.resident_set_plan(None)
        assert state_error(bat.resident_get_plan)
        bat.resident_set_paths(short, RES)   # (reuses the array)
        assert state_error(bat.resident_get_plan)
        x, y = bat.resident_read_path(3)
        assert same(x, short[3][0]) and same(y, short[3][1])

    try:
        lost = memory_shrinks_by(cycle)
    finally:
        bat.close()
    assert lost < BOUND, "device memory shrank by %.1f MiB over %d replacement cycles" % (lost / 2**20, CYCLES)

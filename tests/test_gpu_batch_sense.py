"""GPU tests (-m gpu) of the batch handles' simulated range sensor (ccv_mppi_batch_set_world, _resident_sense_enqueue and their
companions; BatchController.set_world / resident_sense).

The contract: after a call the layer and the float cells of every sensed map are, in every bit, what a fresh _set_occupancy of the
sensed layer would produce, and `first` and `sensor_cell` are the search itself.  The checker is tests/sense_reference.py on top of
tests/scan_reference.py and tests/costmap_reference.py -- integers and one table lookup after one pose-to-cell step -- so
everything is held against it with no tolerance, and a sensing handle against a twin that was given the checker's float map
through _set_grids bit for bit in everything a tick leaves.  The worlds here have a resolution of 2^-2 or 2^-4 and origins that are
multiples of it, so that a pose can be put exactly on a cell edge.  No test asserts a time, and none checks from the host that the
call did not synchronise.  (A straight beam from inside the world leaves it at most once, so "leaves the world and comes back"
cannot happen on the device; beams that leave are here, the sensor outside the world is the checker's own test.)
"""
import ctypes as C

import numpy as np
import pytest

import batch_support as BS
import costmap_reference as CR
import costmap_support as CS
import fleet_support as FS
import grid_reference as GR
import obstacle_cases as OC
import roll_reference as RR
import scan_reference as SR
import sense_reference as SN
from batch_support import GRID, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, batch, capi, configs
from costmap_support import derived, same

pytestmark = pytest.mark.gpu
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
FREE = CR.FREE_VALUE
RES, WORIGIN = 0.25, (-3.0, 1.5)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


@pytest.fixture(scope="module")
def fleet8():
    bat = BatchController(configs.diff_drive_defaults(128, 15), 8)
    bat.resident_set_paths(BS.path_of(0))
    yield bat
    bat.close()


def pose_at(cell, frac=(0.5, 0.5), origin=WORIGIN, res=RES):
    return (origin[0] + (cell[0] + frac[0]) * res, origin[1] + (cell[1] + frac[1]) * res)


def map_at(cells, anchor, threshold=128, origin=WORIGIN, res=RES):
    """set_occupancy's tuple for a map whose cell (0, 0) is the world cell `anchor`"""
    return (cells, (origin[0] + anchor[0] * res, origin[1] + anchor[1] * res), res, CR.OUTSIDE, threshold)


def set_poses(bat, xy):
    st = np.zeros((bat.B, 3))
    st[:len(xy), :2] = np.asarray(xy, dtype=np.float64)
    bat.resident_set_poses(st, np.arange(1, bat.B + 1, dtype=np.uint64))
    return st


class Model:
    """the checker's state of one handle: the layers, the frames, the world and the read-back"""

    def __init__(self, B, layers, thresholds, inflations, map_of, anchors, world, wthr, max_beams, origin=WORIGIN, res=RES):
        self.layers, self.thresholds, self.inflations, self.map_of = [np.array(l, copy=True) for l in layers], thresholds, inflations, map_of
        self.anchors, self.rolled = np.asarray(anchors, dtype=np.int64).reshape(-1, 2), np.zeros((len(layers), 2), dtype=np.int64)
        self.world, self.wthr, self.origin, self.res = np.array(world, copy=True), wthr, origin, res
        self.first, self.cell = np.full((B, max_beams), -1, dtype=np.int32), np.full((B, 2), -1, dtype=np.int32)

    def install(self, bat, weight=1.0, max_beams=None):
        bat.set_occupancy([map_at(l, a, t, self.origin, self.res) for l, a, t in zip(self.layers, self.anchors, self.thresholds)], self.inflations,
                          self.map_of, weight)
        bat.set_world(self.world, self.wthr, self.origin, self.res, self.anchors, self.first.shape[1] if max_beams is None else max_beams)

    def sense(self, instances, beams, poses, clear=0, mark=255):
        wny, wnx = self.world.shape
        for b in instances:
            m = self.map_of[b]
            s = SN.pose_cell(poses[b][0], poses[b][1], self.origin, self.res, wnx, wny)
            self.layers[m], f = SN.apply_sense(self.layers[m], self.anchors[m] + self.rolled[m], self.world, self.wthr, s, beams, clear, mark)
            self.first[b, :len(f)] = f
            self.cell[b] = (-1, -1) if s is None else s

    def cost(self, m):
        R, profile, free = self.inflations[m]
        return CR.cost_separable(self.layers[m], self.thresholds[m], R, profile, free)

    def holds(self, bat, maps=None):
        for m in range(len(self.layers)) if maps is None else maps:
            assert same(bat.read_occupancy(m), self.layers[m]), m
            assert same(derived(bat, m), self.cost(m)), m
        first, cell = bat.resident_read_sense()
        assert same(first, self.first), np.argwhere(first != self.first)[:5]
        assert same(cell, self.cell), (cell, self.cell)


def raw_sense(bat, instances, beams, clear=0, mark=255, expect=capi.OK):
    """the C call over the caller's own arrays, which are overwritten as soon as it returns"""
    inst = np.array(instances, dtype=np.int32)
    table = np.array(beams, dtype=np.int32).reshape(-1, 2).copy()
    rc = bat.lib.ccv_mppi_batch_resident_sense_enqueue(bat._h, len(inst), inst.ctypes.data_as(i32p), len(table), table.ctypes.data_as(i32p), clear, mark)
    assert rc == expect, (rc, bat.lib.ccv_mppi_batch_last_error(bat._h))
    inst[...] = -5
    table[...] = 12345


def mixed_world(wnx, wny, seed=0):
    W = {w[0]: w[1] for w in SN.worlds(wnx, wny, seed)}
    return np.maximum(W["ring"], W["random_0.03"])


# 1. one call from scratch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 3, 17, 64))
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_one_call_equals_the_checker_from_scratch(fleet8, nx, ny, R):
    """six robots on maps of their own sense in one call: one whose pose lies exactly on a cell edge, one in a corner of its map,
    one whose cell lies outside its own map, one outside the world, one with a NaN pose, one whose map hangs over the world's
    edge; a seventh map is not named, an eighth robot has no map.  Then a second call, the entries reversed, other bytes."""
    bat, profile = fleet8, CR.distinct_profile(R)
    wnx, wny = nx + 20, ny + 14
    named = SR.layers(nx, ny)
    layers = [l[1] for l in named] + [named[1][1], named[0][1], named[1][1]]
    thresholds = [l[2] for l in named] + [named[1][2], named[0][2], named[1][2]]
    anchors = [(10, 7)] * 5 + [(-(nx // 2), -1), (10, 7)]
    map_of = np.array([0, 1, 2, 3, 4, 5, 6, -1], dtype=np.int32)
    beams = np.concatenate([SN.fan(96, 0.6 * max(nx, ny) + 3)] + [t for name, t in SN.beam_tables(nx, ny) if name in ("zero_and_one", "octants")])
    model = Model(8, layers, thresholds, [(R, profile, FREE)] * len(layers), map_of, anchors, mixed_world(wnx, wny), 128, len(beams) + 3)
    model.install(bat)
    poses = set_poses(bat, [pose_at((10 + nx // 2, 7 + ny // 2), (0.0, 0.0)), pose_at((10, 7 + ny - 1)), pose_at((8, 7 + ny // 2)),
                            (WORIGIN[0] - 1.0, WORIGIN[1] + 1.0), (np.nan, WORIGIN[1] + 1.0), pose_at((0, min(ny // 2, wny - 1)), (0.0, 0.99)),
                            pose_at((12, 9)), pose_at((12, 9))])
    model.holds(bat)   # (nothing sensed yet: -1 everywhere)
    bat.resident_sense([0, 1, 2, 3, 4, 5], beams)
    model.sense([0, 1, 2, 3, 4, 5], beams, poses)
    assert model.cell[0].tolist() == [10 + nx // 2, 7 + ny // 2] and model.cell[3].tolist() == [-1, -1] and model.cell[4].tolist() == [-1, -1]
    model.holds(bat)
    raw_sense(bat, [5, 4, 3, 2, 1, 0], beams[::-1], clear=1, mark=254)
    model.sense([0, 1, 2, 3, 4, 5], beams[::-1], poses, clear=1, mark=254)
    model.holds(bat)
    assert same(model.layers[6], layers[6]) and same(model.layers[3], layers[3]) and same(model.layers[4], layers[4])


# 2. beam counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 4096))
def test_beam_counts(fleet8, n):
    bat, R, (nx, ny) = fleet8, 3, (130, 70)
    profile = CR.distinct_profile(R)
    layers = [np.full((ny, nx), 100, dtype=np.uint8)]
    model = Model(8, layers, [100], [(R, profile, FREE)], np.array([0] + [-1] * 7, dtype=np.int32), [(10, 7)], mixed_world(nx + 20, ny + 14, seed=n), 128, n)
    model.install(bat)
    poses = set_poses(bat, [pose_at((70, 40))])
    beams = batch.beam_fan(n, 40, phase=0.01 * n)
    bat.resident_sense([0], beams)
    model.sense([0], beams, poses)
    assert (model.first >= 0).any() and (model.layers[0] == 255).any() and (model.layers[0] == 0).any()
    model.holds(bat)
    # one beam more than max_beams is refused, and changes nothing
    raw_sense(bat, [0], np.concatenate([beams, beams[:1]]), expect=capi.ERR_INVALID_ARG)
    if n == 4096:
        with pytest.raises(RuntimeError):
            bat.set_world(model.world, 128, WORIGIN, RES, model.anchors, capi.SENSE_MAX_BEAMS + 1)
    model.holds(bat)


# 3. reaches and blocked cells -----------------------------------------------------------------------------------------------------
def test_reaches_and_blocked_cells(fleet8):
    """a 4097 x 3 world and a map of its size; beams of reach 1, 63, 64, 65, 129 and 4096, of length 0, and beams that leave the
    world; the blocked cell at i = 1, at an end cell, in the second chunk of 64 cells, nowhere -- the world changed by patches
    between the calls"""
    bat, R, (nx, ny) = fleet8, 3, (4097, 3)
    profile = CR.distinct_profile(R)
    beams = np.array([(1, 0), (63, 0), (64, 1), (65, -1), (129, 0), (4096, 1), (4096, 0), (0, 0), (4096, -1), (-5, 0), (3, 4000), (200, -90), (0, 1)],
                     dtype=np.int32)
    model = Model(8, [np.full((ny, nx), 100, dtype=np.uint8)], [100], [(R, profile, FREE)], np.array([0] + [-1] * 7, dtype=np.int32), [(0, 0)],
                  np.zeros((ny, nx), dtype=np.uint8), 7, len(beams))
    model.install(bat)
    poses = set_poses(bat, [pose_at((0, 1))])
    for name, cells in (("nowhere", []), ("at_i_1", [(1, 1)]), ("at_end_cells", [(65, 0), (4096, 2), (4096, 0)]), ("second_chunk", [(100, 1), (70, 2)]),
                        ("first_cell_of_a_chunk", [(64, 1)])):
        world = np.zeros((ny, nx), dtype=np.uint8)
        for x, y in cells:
            world[y, x] = 7
        bat.set_occupancy([map_at(np.full((ny, nx), 100, dtype=np.uint8), (0, 0), 100)], (R, profile, FREE), model.map_of, 1.0)
        bat.set_world(np.zeros((ny, nx), dtype=np.uint8), 7, WORIGIN, RES, [(0, 0)], len(beams))
        bat.update_world(0, 0, world)   # (4097 * 3 cells: one patch)
        model.layers, model.world = [np.full((ny, nx), 100, dtype=np.uint8)], world
        model.first[...], model.cell[...] = -1, -1
        assert same(bat.read_world(), world), name
        bat.resident_sense([0], beams, clear=0, mark=255)
        model.sense([0], beams, poses)
        model.holds(bat)
        f = model.first[0].tolist()
        if name == "nowhere":
            assert f == [-1] * len(beams) and model.layers[0][1, :4096].max() == 0 and model.layers[0][1, 4096] == 100
        if name == "at_i_1":
            assert f[0] == f[1] == f[4] == f[6] == 1 and f[7] == -1 and model.layers[0][1, 1] == 255 and model.layers[0][1, 0] == 0
        if name == "at_end_cells":
            assert f[3] == 65 and f[5] == 4096 and f[8] == 4096 and model.layers[0][2, 4096] == 255 and model.layers[0][0, 65] == 255
        if name == "second_chunk":
            assert f[4] == 100 and f[6] == 100 and model.layers[0][1, 99] == 0 and model.layers[0][1, 100] == 255 and model.layers[0][1, 101] == 100
        if name == "first_cell_of_a_chunk":
            assert f[1] == -1 and f[2] == -1 and f[4] == 64 and f[6] == 64 and model.layers[0][1, 63] == 0 and model.layers[0][1, 64] == 255


# 4. marks and clears --------------------------------------------------------------------------------------------------------------
def test_marks_and_clears_whatever_the_order(fleet8):
    """1 024 beams through one cell, the sensor's right-hand neighbour, which is also the blocked cell of a beam in the middle of
    the table, and 64 beams the other way that nothing blocks; the same beams reversed; two robots with the entries in either order"""
    bat, R, (nx, ny) = fleet8, 3, (200, 150)
    profile = CR.distinct_profile(R)
    s, c = (20, 60), (21, 60)
    far = np.array([(100 + j, k) for j in range(32) for k in range(-16, 16)], dtype=np.int32)
    assert len(far) == 1024 and all((SN.beam_cells(s, d)[1] == c).all() for d in far[::37])
    back = np.array([(-18, k) for k in range(-32, 32)], dtype=np.int32)
    beams = np.concatenate([far[:512], np.array([(1, 0)], dtype=np.int32), far[512:], back])
    world = np.zeros((ny, nx), dtype=np.uint8)
    world[c[1], c[0]] = world[60, 150] = 1
    map_of = np.array([0, 1] + [-1] * 6, dtype=np.int32)
    for table, entries in ((beams, [0, 1]), (beams[::-1].copy(), [0, 1]), (beams, [1, 0])):
        model = Model(8, [np.full((ny, nx), 100, dtype=np.uint8)] * 2, [100, 100], [(R, profile, FREE)] * 2, map_of, [(0, 0), (0, 0)], world, 1, len(beams))
        model.install(bat)
        poses = set_poses(bat, [pose_at(s), pose_at(s)])
        raw_sense(bat, entries, table)
        model.sense(entries, table, poses)
        assert model.layers[0][c[1], c[0]] == 255 and model.layers[0][s[1], s[0]] == 0 and model.layers[0][60, 150] == 100
        assert (model.first[0, :len(beams)] == 1).sum() == 1025 and (model.layers[0] == 0).sum() > 200
        model.holds(bat)


# 5. rolled frames -----------------------------------------------------------------------------------------------------------------
def test_the_beams_land_in_the_rolled_frame(fleet8):
    bat, R, (nx, ny) = fleet8, 17, (67, 45)
    profile = CR.distinct_profile(R)
    rng = np.random.default_rng(5)
    layers = [np.where(rng.random((ny, nx)) < 0.3, 200, 50).astype(np.uint8) for _ in range(2)]
    model = Model(8, layers, [128, 128], [(R, profile, FREE)] * 2, np.array([0, 1] + [-1] * 6, dtype=np.int32), [(5, 4), (9, 2)], mixed_world(100, 70, 3), 128, 200)
    model.install(bat)
    poses = set_poses(bat, [pose_at((40, 30)), pose_at((44, 20))])
    for dx, dy in ((3, -2), (-1, 4)):   # map 0 rolled twice before the call, map 1 never
        bat.roll_occupancy([0], [dx], [dy], fill=77)
        model.layers[0] = RR.roll_layer(model.layers[0], dx, dy, fill=77)
        model.rolled[0] += (dx, dy)
    beams = batch.beam_fan(200, 33, 0.2)
    bat.resident_sense([1, 0], beams)
    model.sense([0, 1], beams, poses)
    model.holds(bat)
    # ... and not in the frame the map was set in
    unrolled, _ = SN.apply_sense(RR.roll_layer(RR.roll_layer(layers[0], 3, -2, fill=77), -1, 4, fill=77), (5, 4), model.world, 128, (40, 30), beams)
    assert not same(unrolled, model.layers[0])


# 6. a changing world --------------------------------------------------------------------------------------------------------------
def test_a_world_patch_between_two_sense_calls(fleet8):
    """sense, a door closes in the world, sense again, a roll, the door opens, sense: no synchronisation in between, every
    array of the caller overwritten as soon as its call returns; everything is read once, at the end"""
    bat, R, (nx, ny) = fleet8, 3, (130, 70)
    profile = CR.distinct_profile(R)
    world = mixed_world(150, 84, 9)
    model = Model(8, [np.full((ny, nx), 100, dtype=np.uint8)] * 2, [100, 100], [(R, profile, FREE)] * 2, np.array([0, 1] + [-1] * 6, dtype=np.int32),
                  [(10, 7), (12, 9)], world, 128, 360)
    model.install(bat)
    bat.roll_occupancy([0, 1], 0, 0)   # the priming call: the roll below allocates nothing
    poses = set_poses(bat, [pose_at((70, 40)), pose_at((60, 45))])
    beams = batch.beam_fan(360, 45)
    ip = lambda a: a.ctypes.data_as(u8p)   # noqa: E731
    raw_sense(bat, [0, 1], beams)
    model.sense([0, 1], beams, poses)
    door = np.full((9, 2), 255, dtype=np.uint8)
    assert bat.lib.ccv_mppi_batch_update_world_enqueue(bat._h, 75, 36, 2, 9, ip(door)) == capi.OK
    door[...] = 0
    model.world = CR.apply_patch(model.world, 75, 36, np.full((9, 2), 255, dtype=np.uint8))
    raw_sense(bat, [1, 0], beams, clear=2, mark=253)
    model.sense([0, 1], beams, poses, clear=2, mark=253)
    assert (model.layers[0][36 - 7:45 - 7, 75 - 10] == 253).any()
    bat.roll_occupancy([0], [4], [-3], fill=9)
    model.layers[0] = RR.roll_layer(model.layers[0], 4, -3, fill=9)
    model.rolled[0] += (4, -3)
    assert bat.lib.ccv_mppi_batch_update_world_enqueue(bat._h, 75, 36, 2, 9, ip(door)) == capi.OK
    door[...] = 255
    model.world = CR.apply_patch(model.world, 75, 36, np.zeros((9, 2), dtype=np.uint8))
    raw_sense(bat, [0], beams[:300], clear=3, mark=252)
    model.sense([0], beams[:300], poses, clear=3, mark=252)
    model.holds(bat)
    assert same(bat.read_world(), model.world) and (model.first[0, 300:] != -1).any()   # (the rows past a call's beams keep the earlier call's)


# 7. the same bits as a twin -------------------------------------------------------------------------------------------------------
TRES = 0.0625
INFLATION = CS.INFLATION


def twin_scene(poses, seed=0, size=(72, 56), home=(20, 28)):
    """a random world round the poses (6 % occupied, cells of 2^-4 m) and per robot an empty map placed from its pose: (world,
    world origin, anchors, the maps of set_occupancy)"""
    poses = np.asarray(poses, dtype=np.float64)
    origin = (float(np.floor(poses[:, 0].min()) - 6.0), float(np.floor(poses[:, 1].min()) - 6.0))
    wnx = int((np.ceil(poses[:, 0].max()) + 6.0 - origin[0]) / TRES)
    wny = int((np.ceil(poses[:, 1].max()) + 6.0 - origin[1]) / TRES)
    rng = np.random.default_rng(seed)
    world = np.where(rng.random((wny, wnx)) < 0.06, 255, 0).astype(np.uint8)
    anchors = []
    for x, y in poses[:, :2]:
        s = SN.pose_cell(x, y, origin, TRES, wnx, wny)
        anchors.append((s[0] - home[0], s[1] - home[1]))
    return world, origin, anchors


def sensed_maps(world, origin, anchors, poses, beams, size=(72, 56)):
    """(set_occupancy's maps before the sensing, the checker's float maps after it as set_grids takes them)"""
    R, profile, free = INFLATION
    wny, wnx = world.shape
    occ, flt = [], []
    for a, (x, y) in zip(anchors, np.asarray(poses)[:, :2]):
        empty = np.zeros((size[1], size[0]), dtype=np.uint8)
        new, first = SN.apply_sense(empty, a, world, 128, SN.pose_cell(x, y, origin, TRES, wnx, wny), beams)
        assert not same(new, empty) and (first >= 0).any()
        occ.append(map_at(empty, a, 128, origin, TRES))
        flt.append((CR.cost_separable(new, 128, R, profile, free),) + occ[-1][1:4])
    return occ, flt


@pytest.mark.parametrize("shift,discs", [(False, "none"), (True, "none"), (False, "moving"), (True, "static")])
def test_a_sensing_handle_gives_the_bits_of_a_twin(shift, discs):
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    inputs = BS.instance_inputs(p, B)
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    beams = batch.beam_fan(180, 22, 0.1)
    world, origin, anchors = twin_scene(x0[[1, 2], :2])
    occ, flt = sensed_maps(world, origin, anchors, x0[[1, 2]], beams)
    d = OC.discs_for(p, inputs, ns=(32, 0, 3, 3, 32)) if discs != "none" else None
    vels = [np.stack([0.3 * np.cos(np.arange(len(a)) + b), 0.2 * np.sin(np.arange(len(a)) - b)], axis=1).reshape(-1, 2)
            for b, a in enumerate(d)] if discs == "moving" else None
    s0, rseeds = BS.start_poses(p, B)
    rworld, rorigin, ranchors = twin_scene(s0[[1, 2], :2], seed=7)
    rocc, rflt = sensed_maps(rworld, rorigin, ranchors, s0[[1, 2]], beams)
    out = []
    for source in ("sensed", "grids"):
        bat = BatchController(p, B, min_shift=shift)
        bat.resident_set_paths([BS.path_of(b) for b in range(B)])
        if d is not None:
            bat.set_obstacles(d, OC.W_OBS, velocities=vels)
        if source == "sensed":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            bat.set_world(world, 128, origin, TRES, anchors, 256)
            bat.resident_set_poses(x0[:, :3], rseeds)   # (the sensor's poses: those the iteration below is given)
            bat.set_nominal(nom)
            bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)   # (a tick over the maps before the sensing)
            k0 = bat.last_kernel()
            bat.resident_sense([1, 2], beams)
            assert bat.last_kernel() == k0
        else:
            bat.set_grids(flt, map_of, w)
        bat.set_nominal(nom)
        u, st = bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0)
        res = [BS.snapshot(bat, u, st), bat.last_kernel(), derived(bat, 0), derived(bat, 1)]
        # five resident ticks over maps placed from the start poses; no step is needed before the sensing
        bat.resident_set_poses(s0, rseeds)
        if source == "sensed":
            bat.set_occupancy(rocc, INFLATION, map_of, w)
            bat.set_world(rworld, 128, rorigin, TRES, ranchors, 180)
            bat.resident_sense([2, 1], beams)
        else:
            bat.set_grids(rflt, map_of, w)
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(CS.tick_bits(bat) + [r.tobytes() for r in bat.resident_read()[:2]] + [bat.resident_read_trace(b).tobytes() for b in range(B)])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    a, b = out
    assert a[1] == b[1] == a[-1] == b[-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | (SHIFT if shift else 0)
    assert same(a[2], b[2]) and same(a[3], b[3]) and len(np.unique(a[2])) > 5
    assert all(BS.same_bits(x, y) for x, y in zip(a[0], b[0]))
    for it in range(5):
        assert a[4 + it] == b[4 + it], it


def test_a_sensing_handle_gives_the_bits_of_a_twin_beside_the_fleet_term():
    p = FS.params("diff_drive", 1000, 15)
    B = 5
    s0, seeds, paths = FS.fleet_start(p, B)
    map_of, w = np.array([-1, 0, 1, 0, 1], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.0, 0.025])
    beams = batch.beam_fan(180, 22, 0.1)
    world, origin, anchors = twin_scene(s0[[1, 2], :2], seed=3)
    occ, flt = sensed_maps(world, origin, anchors, s0[[1, 2]], beams)
    static = [FS.far_discs(b % 3, b) for b in range(B)]
    out = []
    for source in ("sensed", "grids"):
        bat = FS.make(p, B, True, static, 50.0, paths, s0, seeds, fleet=(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0)))
        bat.resident_set_fleet_prediction(True)
        if source == "sensed":
            bat.set_occupancy(occ, INFLATION, map_of, w)
            bat.set_world(world, 128, origin, TRES, anchors, 180)
            bat.resident_sense([1, 2], beams)
        else:
            bat.set_grids(flt, map_of, w)
        res = []
        for it in range(5):
            bat.resident_step_enqueue(p.dt, it, advance=it > 0)
            res.append(CS.tick_bits(bat) + [bat.resident_read()[0].tobytes()])
        res.append(bat.last_kernel())
        bat.close()
        out.append(res)
    assert out[0] == out[1] and out[0][-1] == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT


# 8. stream order ------------------------------------------------------------------------------------------------------------------
T_STREAM = 30


def test_sensing_takes_effect_in_stream_order():
    """A: occupancy and a world; after every resident step one sense call of both robots and a roll of robot 0's map that brings
    the robot back to its home cell, and nothing else between the steps.  B: before every step the checker's full maps of that
    moment through _set_grids.  B runs first, tick by tick: it reads the poses, runs the checker and decides the rolls.  The world
    is 6 % occupied and the beams reach 11 cells, about as far as the rollouts, so that what a robot discovers lies where its
    next candidates go.  At least a third of the sense calls must change the cost of a cell that some covered state of the next
    tick reads (on B's read-back candidates; A's are the same bits); the test fails there, before A runs, if the scene does not
    qualify."""
    p = configs.diff_drive_defaults(128, 15)
    B, R = 2, 3
    profile, free = CR.distinct_profile(R) * np.float32(0.001), 0.0
    s0, seeds = BS.start_poses(p, B)
    paths = [BS.path_of(b) for b in range(B)]
    sizes, home = [(64, 48), (97, 95)], (24, 24)
    world, origin, _ = twin_scene(s0[:, :2], seed=11)
    wny, wnx = world.shape
    cell0 = [SN.pose_cell(s0[b, 0], s0[b, 1], origin, TRES, wnx, wny) for b in range(B)]
    anchors = np.array([(cell0[0][0] - home[0], cell0[0][1] - home[1]), (cell0[1][0] - 48, cell0[1][1] - 47)], dtype=np.int64)
    map_of, w = np.array([0, 1], dtype=np.int32), np.array([0.5, 0.3])
    beams = batch.beam_fan(120, 11)
    origin0 = [(origin[0] + a[0] * TRES, origin[1] + a[1] * TRES) for a in anchors]

    def result(bat):
        return [bat.get_nominal().tobytes(), bat.read_costs(0).tobytes(), bat.read_costs(1).tobytes(), bat.resident_read()[0].tobytes(),
                bat.resident_read_trace(0).tobytes(), bat.resident_read_trace(1).tobytes()]

    def world_keys(geo_origin_cells, idx, nx):
        iy, ix = np.divmod(idx, nx)
        return (ix + geo_origin_cells[0]) * 65536 + (iy + geo_origin_cells[1])

    # B: the reference handle, which also decides the rolls
    layers = [np.zeros((ny, nx), dtype=np.uint8) for nx, ny in sizes]
    cost = [CR.cost_separable(l, 128, R, profile, free) for l in layers]
    rolled = np.zeros((B, 2), dtype=np.int64)
    ref = BatchController(p, B, min_shift=True)
    ref.resident_set_paths(paths)
    ref.resident_set_poses(s0, seeds)
    rolls, changed, looked_at = [], None, 0
    for it in range(T_STREAM):
        origins = [RR.rolled_origin(origin0[m], tuple(int(v) for v in rolled[m]), TRES) for m in range(B)]
        ref.set_grids([(cost[m], origins[m], TRES, 0.0) for m in range(B)], map_of, w)
        ref.resident_step_enqueue(p.dt, it, advance=it > 0)
        read = []
        for b in range(B):
            geo = GR.Grid(cost[b], origins[b], TRES, 0.0)
            idx = CS.cells_hit(geo, ref.read_candidates(b)[:, :GR.n_covered(p.model, p.horizon)])
            read.append(world_keys(anchors[b] + rolled[b], idx, sizes[b][0]))
        if changed is not None:
            looked_at += bool(np.intersect1d(np.concatenate(read), changed).size)
        pose = ref.resident_read()[0]
        keys = []
        for b in range(B):
            s = SN.pose_cell(pose[b, 0], pose[b, 1], origin, TRES, wnx, wny)
            layers[b], _ = SN.apply_sense(layers[b], anchors[b] + rolled[b], world, 128, s, beams)
            new = CR.cost_separable(layers[b], 128, R, profile, free)
            keys.append(world_keys(anchors[b] + rolled[b], np.flatnonzero(new.reshape(-1) != cost[b].reshape(-1)), sizes[b][0]))
            cost[b] = new
        changed = np.concatenate(keys)
        s = SN.pose_cell(pose[0, 0], pose[0, 1], origin, TRES, wnx, wny)
        d = (int(s[0] - anchors[0][0] - rolled[0][0] - home[0]), int(s[1] - anchors[0][1] - rolled[0][1] - home[1]))
        rolls.append(d)
        layers[0] = RR.roll_layer(layers[0], d[0], d[1], fill=0)
        rolled[0] += d
        cost[0] = CR.cost_separable(layers[0], 128, R, profile, free)
    want, k_ref = result(ref), ref.last_kernel()
    ref.close()
    print("[stream order] %d of %d sense calls changed a cell that the next tick read; %d rolls moved the map"
          % (looked_at, T_STREAM - 1, sum(1 for d in rolls if d != (0, 0))))
    assert 3 * looked_at >= T_STREAM and any(d != (0, 0) for d in rolls)
    # A: occupancy and the world, sensed and rolled in stream order
    bat = BatchController(p, B, min_shift=True)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    bat.set_occupancy([map_at(np.zeros((ny, nx), dtype=np.uint8), a, 128, origin, TRES)[:3] + (0.0, 128) for (nx, ny), a in zip(sizes, anchors)],
                      (R, profile, free), map_of, w)
    bat.set_world(world, 128, origin, TRES, anchors, len(beams))
    bat.roll_occupancy([0, 1], 0, 0)   # the priming call
    for it in range(T_STREAM):
        bat.resident_step_enqueue(p.dt, it, advance=it > 0)
        raw_sense(bat, [0, 1], beams)
        bat.roll_occupancy([0], [rolls[it][0]], [rolls[it][1]], fill=0)
    got = result(bat)
    assert bat.last_kernel() == k_ref == capi.BATCH_KERNEL_FOUR_WAVE | GRID | SHIFT
    for m in range(B):
        assert same(bat.read_occupancy(m), layers[m]) and same(derived(bat, m), cost[m]), m
    bat.close()
    assert got == want


# 9. plumbing ----------------------------------------------------------------------------------------------------------------------
def plumbing_scene():
    p = configs.diff_drive_defaults(1000, 15)
    B = 5
    s0, seeds = BS.start_poses(p, B)
    map_of, w = np.array([-1, 0, 1, 0, 2], dtype=np.int32), np.array([0.0, 0.01, 0.01, 0.02, 0.025])
    beams = batch.beam_fan(180, 22, 0.1)
    world, origin, anchors = twin_scene(s0[[1, 2, 4], :2], seed=5)
    occ, _ = sensed_maps(world, origin, anchors, s0[[1, 2, 4]], beams)
    return p, B, s0, seeds, map_of, w, beams, world, origin, anchors, occ


def test_refusals_change_nothing_and_the_setters_keep_or_drop_the_world():
    p, B, s0, seeds, map_of, w, beams, world, origin, anchors, occ = plumbing_scene()
    bat = BatchController(p, B)
    lib, ip = bat.lib, lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(i32p)   # noqa: E731
    wrow = capi.Occupancy(origin[0], origin[1], TRES, 0.0, world.shape[1], world.shape[0], 128, world.ctypes.data_as(u8p))
    flat = np.ascontiguousarray(np.asarray(anchors, dtype=np.int32))

    def set_world(row=wrow, a=flat, mb=200):
        return lib.ccv_mppi_batch_set_world(bat._h, C.byref(row) if row is not None else None, ip(a) if a is not None else None, mb)

    # no occupancy: no world; no world: no sensing, no read-back
    assert set_world() == capi.ERR_STATE
    raw_sense(bat, [1], beams, expect=capi.ERR_STATE)
    assert lib.ccv_mppi_batch_resident_read_sense(bat._h, None, None) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_get_world(bat._h, None, None, 0, None) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_read_world(bat._h, world.ctypes.data_as(u8p)) == capi.ERR_STATE
    assert lib.ccv_mppi_batch_update_world_enqueue(bat._h, 0, 0, 1, 1, world.ctypes.data_as(u8p)) == capi.ERR_STATE
    assert set_world(None, None, 0) == capi.OK   # (dropping no world)
    bat.set_occupancy(occ, INFLATION, map_of, w)
    # what _set_world refuses
    def row(**kw):
        r = capi.Occupancy(origin[0], origin[1], TRES, 0.0, world.shape[1], world.shape[0], 128, world.ctypes.data_as(u8p))
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    far = flat.copy()
    far[1, 0] = 2 ** 29 + 1
    for args in ((row(nx=0),), (row(ny=32769),), (row(origin_x=np.inf),), (row(resolution=np.nan),), (row(resolution=0.0),),
                 (row(threshold=256),), (row(threshold=-1),), (row(cells=None),), (wrow, None), (wrow, flat, 0), (wrow, flat, capi.SENSE_MAX_BEAMS + 1),
                 (wrow, far), (wrow, -far)):
        assert set_world(*args) == capi.ERR_INVALID_ARG, args
    assert lib.ccv_mppi_batch_get_world(bat._h, None, None, 0, None) == capi.ERR_STATE
    # no poses: no sensing
    assert set_world() == capi.OK
    raw_sense(bat, [1], beams, expect=capi.ERR_STATE)
    bat.resident_set_paths([BS.path_of(b) for b in range(B)])
    raw_sense(bat, [1], beams, expect=capi.ERR_STATE)
    bat.resident_set_poses(s0, seeds)
    (o, res, wnx, wny, thr, got_anchors, mb) = bat.get_world()
    assert (o, res, wnx, wny, thr, mb) == (origin, TRES, world.shape[1], world.shape[0], 128, 200) and same(got_anchors, flat)
    assert same(bat.read_world(), world)
    assert lib.ccv_mppi_batch_get_world(bat._h, None, ip(np.zeros(4)), 2, None) == capi.ERR_INVALID_ARG

    def tick():
        bat.resident_set_poses(s0, seeds)
        bat.set_nominal(np.zeros((B, p.horizon - 1, p.udim)))
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        return CS.tick_bits(bat)

    def state():
        first, cell = bat.resident_read_sense()
        return [bat.read_occupancy(m).tobytes() + derived(bat, m).tobytes() for m in range(3)] + [first.tobytes(), cell.tobytes(), bat.read_world().tobytes()]

    bat.resident_sense([1, 2], beams)
    before, bits = state(), tick()
    # every refusal of the sensing and of the world patch
    reach = capi.SCAN_MAX_REACH + 1
    for inst, table, clear, mark in (([], beams, 0, 255), ([0, 1, 2, 3, 4, 1], beams, 0, 255), ([5], beams, 0, 255), ([-1], beams, 0, 255), ([1, 1], beams, 0, 255),
                                     ([0], beams, 0, 255), ([1, 3], beams, 0, 255), ([3, 2, 1], beams, 0, 255), ([1], beams[:0], 0, 255),
                                     ([1], np.resize(beams, (201, 2)), 0, 255), ([1], [(reach, 0)], 0, 255), ([1], [(0, 0), (3, -reach)], 0, 255),
                                     ([1], [(-2 ** 31, 2 ** 31 - 1)], 0, 255), ([1], beams, -1, 255), ([1], beams, 256, 255), ([1], beams, 0, -1), ([1], beams, 0, 256)):
        raw_sense(bat, inst, table, clear, mark, expect=capi.ERR_INVALID_ARG)
    call = lib.ccv_mppi_batch_resident_sense_enqueue
    assert call(bat._h, 1, None, 2, ip(beams[:2]), 0, 255) == capi.ERR_INVALID_ARG and call(bat._h, 1, ip([1]), 2, None, 0, 255) == capi.ERR_INVALID_ARG
    patch = np.full(4, 255, dtype=np.uint8)
    for x0, y0, pw, ph in ((-1, 0, 2, 2), (0, -1, 2, 2), (world.shape[1] - 1, 0, 2, 2), (0, world.shape[0] - 1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0)):
        assert lib.ccv_mppi_batch_update_world_enqueue(bat._h, x0, y0, pw, ph, patch.ctypes.data_as(u8p)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_update_world_enqueue(bat._h, 0, 0, 2, 2, None) == capi.ERR_INVALID_ARG
    assert state() == before and tick() == bits
    # a map of another resolution: named alone it is refused, the others still sense
    other = list(occ)
    other[2] = occ[2][:2] + (TRES * 2,) + occ[2][3:]
    bat.set_occupancy(other, INFLATION, map_of, w)
    assert lib.ccv_mppi_batch_get_world(bat._h, None, None, 0, None) == capi.ERR_STATE   # (_set_occupancy dropped the world)
    assert set_world() == capi.OK
    raw_sense(bat, [4], beams, expect=capi.ERR_INVALID_ARG)
    raw_sense(bat, [1, 4], beams, expect=capi.ERR_INVALID_ARG)
    raw_sense(bat, [1, 2], beams)
    # an accumulated frame offset beyond 2^30: the anchor at its limit, and rolls of the largest step until the sum passes it
    bat.set_occupancy(occ, INFLATION, map_of, w)
    edge = flat.copy()
    edge[0] = (2 ** 29, -5)
    assert set_world(wrow, edge) == capi.OK
    bat.roll_occupancy([0], 0, 0)
    for _ in range(2 ** 29 // 32768):
        bat.roll_occupancy([0], [32768], [0])
    raw_sense(bat, [1], beams)   # (2^30 exactly: legal, and nothing of the map in reach)
    bat.roll_occupancy([0], [1], [0])
    raw_sense(bat, [1], beams, expect=capi.ERR_INVALID_ARG)
    raw_sense(bat, [2, 3], beams, expect=capi.ERR_INVALID_ARG)
    raw_sense(bat, [2], beams)
    assert bat.resident_read_sense()[1][1].tolist() == list(SN.pose_cell(s0[1, 0], s0[1, 1], origin, TRES, world.shape[1], world.shape[0]))
    # the other setters keep world, anchors and read-back
    bat.set_occupancy(occ, INFLATION, map_of, w)
    assert set_world() == capi.OK
    bat.resident_sense([1, 2], beams)
    assert state() == before
    inputs = BS.instance_inputs(p, B)
    discs = OC.discs_for(p, inputs, ns=(0, 3, 0, 3, 0))
    bat.set_params([p] * B)
    bat.set_params(None)
    bat.set_obstacles(discs, OC.W_OBS, velocities=[np.zeros((len(a), 2)) for a in discs])
    bat.set_obstacle_velocities(None)
    bat.set_obstacles(None)
    bat.set_min_shift(True)
    bat.set_min_shift(False)
    bat.resident_set_fleet(np.full(B, 0.25), 3.0, 4, np.full(B, 50.0))
    bat.resident_set_fleet(None)
    bat.resident_set_poses(s0, seeds)
    assert state() == before and same(bat.get_world()[5], flat) and bat.get_world()[6] == 200
    bat.resident_sense([1, 2], beams)   # (sensing what is sensed already changes nothing)
    assert state() == before and tick() == bits
    # _set_grids and _set_world(NULL) drop the world
    bat.set_world(None)
    assert lib.ccv_mppi_batch_get_world(bat._h, None, None, 0, None) == capi.ERR_STATE
    assert set_world() == capi.OK
    bat.set_grids([(derived(bat, m),) + occ[m][1:4] for m in range(3)], map_of, w)
    assert lib.ccv_mppi_batch_get_world(bat._h, None, None, 0, None) == capi.ERR_STATE
    raw_sense(bat, [1], beams, expect=capi.ERR_STATE)
    assert set_world() == capi.ERR_STATE
    bat.close()


def test_one_instances_sensing_changes_no_bit_of_an_instance_on_another_map():
    p, B, s0, seeds, map_of, w, beams, world, origin, anchors, occ = plumbing_scene()
    j = 2   # (instance 2 alone is on map 1)
    snaps = []
    for sensed in (False, True):
        bat = BatchController(p, B, min_shift=True)
        bat.resident_set_paths([BS.path_of(b) for b in range(B)])
        bat.resident_set_poses(s0, seeds)
        bat.set_occupancy(occ, INFLATION, map_of, w)
        bat.set_world(world, 128, origin, TRES, anchors, 180)
        if sensed:
            bat.resident_sense([j], beams)
        bat.resident_step_enqueue(p.dt, 0, advance=False)
        snaps.append([bat.get_nominal()] + [(bat.read_costs(b), bat.read_weights(b), bat.read_candidates(b)) for b in range(B)] +
                     [bat.resident_read_sense()])
        bat.close()
    assert not np.array_equal(snaps[0][1 + j][0], snaps[1][1 + j][0])
    for b in range(B):
        if b != j:
            assert same(snaps[0][0][b], snaps[1][0][b]) and all(same(x, y) for x, y in zip(snaps[0][1 + b], snaps[1][1 + b])), b
    first0, first1 = snaps[0][-1][0], snaps[1][-1][0]
    assert (first0 == -1).all() and (first1[j] >= 0).any() and (np.delete(first1, j, axis=0) == -1).all()


def test_the_world_returns_all_device_and_pinned_memory():
    import torch
    p = configs.diff_drive_defaults(1000, 15)
    B = 16
    map_of, w = np.arange(B, dtype=np.int32) % 2, np.full(B, 0.01)
    big = (np.ones((700, 900), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    small = (np.ones((3, 5), dtype=np.uint8), (0.0, 0.0), 0.05, 0.0, 1)
    infl = batch.inflation_profile(0.5, 0.05)
    world = np.zeros((3000, 4000), dtype=np.uint8)
    world[::7, ::5] = 1
    beams = batch.beam_fan(360, 250)
    s0 = np.zeros((B, 3))
    s0[:, 0], s0[:, 1] = 20.0 + np.arange(B), 15.0

    def level():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        bat = BatchController(p, B)
        bat.resident_set_paths(BS.path_of(0))
        bat.resident_set_poses(s0, 1)
        bat.set_occupancy([big, small], infl, map_of, w)
        bat.set_world(world, 1, (0.0, 0.0), 0.05, [(0, 0), (400, 300)], 4096)
        for _ in range(capi.OCC_PATCH_SLOTS + 1):
            bat.resident_sense([0, 1], beams)
        bat.set_world(world[:100, :100], 1, (0.0, 0.0), 0.05, [(0, 0), (400, 300)], 360)   # (a new world takes the old one's place)
        bat.resident_sense([2], beams)
        bat.set_world(None)
        bat.set_world(world, 1, (0.0, 0.0), 0.05, [(0, 0), (400, 300)], 4096)
        bat.set_occupancy(None)   # (drops the world with the layers)
        bat.set_occupancy([big, small], infl, map_of, w)
        bat.set_world(world, 1, (0.0, 0.0), 0.05, [(0, 0), (400, 300)], 4096)
        bat.close()               # (... and so does destroy)

    for _ in range(3):   # runtime pools settle
        cycle()
    free0, rss0 = level(), CS._rss_kb()
    for _ in range(40):
        cycle()
    free1, rss1 = level(), CS._rss_kb()
    assert free0 - free1 < 8 * 2**20, "device memory shrank by %.1f MiB over 40 cycles" % ((free0 - free1) / 2**20)
    assert rss1 - rss0 < 96 * 1024, "resident host memory grew by %d kB over 40 cycles" % (rss1 - rss0)

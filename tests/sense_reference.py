"""Range sensors simulated on the device (ccv_mppi_batch_resident_sense_enqueue), restated on top of
scan_reference.py and costmap_reference.py.

The spec, integers only after one pose-to-cell step.  With `world` the ground truth, s the robot's world cell, (dx, dy) a beam's
end offset and (off_x, off_y) = anchor + rolled cells the world cell of the map's cell (0, 0):

    fx = (x - origin_x) * inv, fy likewise, inv = RN(1 / resolution);  in = 0 <= fx < nx and 0 <= fy < ny;  s = (int(fx), int(fy))
    the beam's cells i = 0 .. a: scan_reference's closed form from s to s + (dx, dy), cell a being the end cell
    f = min { i in [1, a] : cell i inside the world and world[cell i] >= threshold }
    local cell = world cell - (off_x, off_y)
    f exists: the local cells of i in [0, f) = clear, then local cell f = mark;  else the local cells of i in [0, a) = clear
    cost = the transform of costmap_reference.py over the new layer, complete

`pose_cell` is the first line, `beam_cells` the second, `first_blocked` the third, `apply_sense` the rest but the cost;
`sense_rect` the one rectangle of float cells an entry derives again (the box s_local + [min dx, max dx] x [min dy, max dy]
clipped to the map, grown by R and clipped again, the extent taken
over the beams and the offset (0, 0)); `sense_cost` that path as a model with its margins as parameters.
tests/test_sense_reference.py holds the model equal to cost_separable(apply_sense(...)) in every bit.  `wrong` names a
deliberately wrong version, for that test.
"""
import numpy as np

import costmap_reference as CR
import scan_reference as SR

MAX_BEAMS = 4096   # CCV_MPPI_SENSE_MAX_BEAMS
WRONG = ("sensor_tested", "end_not_tested", "outside_occupied", "blocked_cleared", "marks_first", "retraced", "wrapped")   # values of `wrong`


def pose_cell(x, y, origin, resolution, nx, ny):
    """the world cell (sx, sy) of the pose, or None where the robot senses nothing (outside the world, or not a number)"""
    inv = 1.0 / float(resolution)
    fx, fy = (np.float64(x) - np.float64(origin[0])) * inv, (np.float64(y) - np.float64(origin[1])) * inv
    if not (fx >= 0.0 and fx < nx and fy >= 0.0 and fy < ny):
        return None
    return int(fx), int(fy)


def beam_cells(s, d):
    """int64 [a + 1][2]: the cells i = 0 .. a of the beam with end offset d from the cell s; the last one is s + d"""
    e = (int(s[0]) + int(d[0]), int(s[1]) + int(d[1]))
    return np.concatenate([SR.ray_cells(s, e), np.array([e], dtype=np.int64)])


def first_blocked(world, threshold, s, d, wrong=None):
    """f: the first i in [1, a] whose cell lies inside the world and is occupied, or -1"""
    wny, wnx = world.shape
    c = beam_cells(s, d)
    a = len(c) - 1
    x, y = c[:, 0], c[:, 1]
    inside = (x >= 0) & (x < wnx) & (y >= 0) & (y < wny)
    occ = np.zeros(a + 1, dtype=bool)
    occ[inside] = world[y[inside], x[inside]] >= threshold
    if wrong == "outside_occupied":
        occ |= ~inside
    if wrong != "sensor_tested":
        occ[0] = False
    if wrong == "end_not_tested" and a >= 1:
        occ[a] = False
    if a == 0:
        return -1
    hit = np.flatnonzero(occ)
    return int(hit[0]) if len(hit) else -1


def apply_sense(layer, offset, world, threshold, s, beams, clear=0, mark=255, wrong=None):
    """(new layer, first int32 [n_beams]) after one robot at world cell s (None: nothing sensed) has cast `beams` int [n][2];
    offset: the world cell of the layer's cell (0, 0)"""
    layer = np.asarray(layer)
    assert layer.dtype == np.uint8 and layer.ndim == 2 and world.dtype == np.uint8
    beams = np.asarray(beams, dtype=np.int64).reshape(-1, 2)
    assert 1 <= len(beams) <= MAX_BEAMS and np.abs(beams).max() <= SR.MAX_REACH
    first = np.full(len(beams), -1, dtype=np.int32)
    new = layer.copy()
    if s is None:
        return new, first
    off = np.asarray(offset, dtype=np.int64)
    clears, marks = [np.zeros((0, 2), dtype=np.int64)], [np.zeros((0, 2), dtype=np.int64)]
    for r, d in enumerate(beams):
        f = first_blocked(world, threshold, s, d, wrong)
        first[r] = f
        c = beam_cells(s, d)
        if f < 0:
            clears.append(c[:-1])
            continue
        if wrong == "retraced":   # scan_reference's line from s to the blocked cell, not the beam's own
            clears.append(SR.ray_cells(s, c[f]))
        else:
            clears.append(c[:f + 1] if wrong == "blocked_cleared" else c[:f])
        if wrong != "blocked_cleared":   # (cleared in place of marked: cleared and then marked would be no different)
            marks.append(c[[f]])
    clears, marks = np.concatenate(clears) - off, np.concatenate(marks) - off
    if wrong == "marks_first":
        SR._put(new, marks, mark)
    SR._put(new, clears, clear, wrap=wrong == "wrapped")
    if wrong != "marks_first":
        SR._put(new, marks, mark, wrap=wrong == "wrapped")
    return new, first


def sense_box(nx, ny, s_local, beams, with_sensor=True):
    """(x0, y0, w, h): s_local + [min dx, max dx] x [min dy, max dy] clipped to the map (w or h 0: it misses the map), min and max
    over the beam table and the offset (0, 0): the box holds the sensor cell and every end cell.  with_sensor=False: over the
    beam table alone."""
    beams = np.asarray(beams, dtype=np.int64).reshape(-1, 2)
    if with_sensor:
        beams = np.concatenate([beams, np.zeros((1, 2), dtype=np.int64)])
    lo, hi = beams.min(axis=0), beams.max(axis=0)
    x0, y0 = max(int(s_local[0] + lo[0]), 0), max(int(s_local[1] + lo[1]), 0)
    x1, y1 = min(int(s_local[0] + hi[0]) + 1, nx), min(int(s_local[1] + hi[1]) + 1, ny)
    return x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)


def sense_rect(nx, ny, s_local, beams, R, grow=None):
    """the rectangle of float cells the entry derives again: sense_box grown by `grow` (default R) and clipped again; a robot that
    senses nothing (s_local None) and a box that misses the map give an empty one, (0, 0, 0, 0)"""
    if s_local is None:
        return 0, 0, 0, 0
    box = sense_box(nx, ny, s_local, beams)
    if box[2] == 0 or box[3] == 0:
        return 0, 0, 0, 0
    return CR.dilated_rect(box, R if grow is None else grow, nx, ny)


def sense_cost(cost_old, layer_new, s_local, beams, threshold, R, profile, free_value, grow=None, reach=None, box=None):
    """The sense path as a model: cost_old with sense_rect derived again from layer_new, looking only at occupancy within
    `reach` (default 2R) of the box; every other cell kept.  box: another box in place of sense_box (a wrong one)."""
    ny, nx = layer_new.shape
    if s_local is None:
        return np.array(cost_old, dtype=np.float32, copy=True)
    box = sense_box(nx, ny, s_local, beams) if box is None else box
    if box[2] == 0 or box[3] == 0:
        return np.array(cost_old, dtype=np.float32, copy=True)
    return CR.patch_cost(cost_old, layer_new, box, threshold, R, profile, free_value, dilate=R if grow is None else grow, reach=reach)


def sense_vectorised(world, threshold, s, beams):
    """first int32 [n_beams] by one vectorised pass over all beams' cells (what a host would run per robot and tick)"""
    beams = np.asarray(beams, dtype=np.int64).reshape(-1, 2)
    wny, wnx = world.shape
    adx, ady = np.abs(beams[:, 0]), np.abs(beams[:, 1])
    xmajor = adx >= ady
    a, b = np.where(xmajor, adx, ady), np.where(xmajor, ady, adx)
    sgx, sgy = np.where(beams[:, 0] < 0, -1, 1), np.where(beams[:, 1] < 0, -1, 1)
    i = np.arange(int(a.max()) + 1, dtype=np.int64)[None, :]
    minor = (2 * i * b[:, None] + a[:, None]) // np.maximum(2 * a[:, None], 1)
    x = s[0] + sgx[:, None] * np.where(xmajor[:, None], i, minor)
    y = s[1] + sgy[:, None] * np.where(xmajor[:, None], minor, i)
    ok = (i >= 1) & (i <= a[:, None]) & (x >= 0) & (x < wnx) & (y >= 0) & (y < wny)
    occ = np.zeros(x.shape, dtype=bool)
    occ[ok] = world[y[ok], x[ok]] >= threshold
    return np.where(occ.any(axis=1), occ.argmax(axis=1), -1).astype(np.int32)


# ---- the cases of the CPU test and of the GPU test -------------------------------------------------------------------------------
def fan(n, reach, phase=0.0):
    """int32 [n][2]: batch.beam_fan restated"""
    t = phase + 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.stack([np.rint(reach * np.cos(t)), np.rint(reach * np.sin(t))], axis=1).astype(np.int32)


def worlds(wnx, wny, seed=0):
    """[(name, cells, threshold)]: empty, a ring of walls two cells inside the border, 3 % random, full"""
    rng = np.random.default_rng(seed)
    ring = np.zeros((wny, wnx), dtype=np.uint8)
    if wnx > 6 and wny > 6:
        ring[2, 2:-2] = ring[-3, 2:-2] = 200
        ring[2:-2, 2] = ring[2:-2, -3] = 200
    return [("empty", np.zeros((wny, wnx), dtype=np.uint8), 1), ("ring", ring, 128),
            ("random_0.03", (rng.random((wny, wnx)) < 0.03).astype(np.uint8) * 255, 255), ("full", np.full((wny, wnx), 9, dtype=np.uint8), 9)]


def beam_tables(nx, ny):
    """[(name, beams)]: a 96-beam fan, a short fan of few beams, beams of length 0 and 1, one beam, the eight octant edges"""
    far = 0.6 * max(nx, ny) + 3
    return [("fan", fan(96, far)), ("short", fan(7, 2.4, 0.3)), ("zero_and_one", np.array([(0, 0), (1, 0), (0, -1), (0, 0)], dtype=np.int32)),
            ("one", np.array([(int(far), 3)], dtype=np.int32)),
            ("octants", np.array([(9, 0), (9, 9), (0, 9), (-9, 9), (-9, 0), (-9, -9), (0, -9), (9, -9), (9, 4), (4, 9)], dtype=np.int32))]


def placements(nx, ny, wnx, wny):
    """[(name, offset, s)]: the map in the middle of the world with the robot at its centre, the robot in a map corner, the robot's
    cell outside its own map, the map hanging over the world's edge, a robot that senses nothing"""
    ox, oy = (wnx - nx) // 2, (wny - ny) // 2
    return [("centre", (ox, oy), (ox + nx // 2, oy + ny // 2)), ("corner", (ox, oy), (ox, oy + ny - 1)),
            ("outside_map", (ox, oy), (max(ox - 2, 0), oy + ny // 2)), ("over_edge", (-(nx // 2), -1), (0, min(ny // 2, wny - 1))),
            ("nothing", (ox, oy), None)]

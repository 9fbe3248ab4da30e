"""Range scans traced into costmaps (ccv_mppi_batch_scan_occupancy_enqueue), restated on top of
costmap_reference.py.

The spec, integers only.  With (sx, sy) the sensor's cell and (ex, ey) a ray's end cell:

    adx = |ex - sx|, ady = |ey - sy|;  the major axis is x if adx >= ady, else y;  a = major length, b = minor length
    cell i, 0 <= i < a:  major = s_major + sign_major * i,  minor = s_minor + sign_minor * ((2 * i * b + a) div (2 * a))
    new = old;  every ray cell inside the map = clear;  then every end cell inside the map of a ray with hit != 0 = mark
    cost = the transform of costmap_reference.py over `new`, complete

`ray_cells` is the closed form, vectorised; `ray_cells_walk` the integer error walk it is the per-step form of; `apply_scan` the
third line; `scan_rect` the one rectangle of float cells an entry derives again (the bounding box of the sensor cell and all end
cells, clipped to the map, grown by R and clipped again); `scan_cost` that path as a model: the old cost with the rectangle taken
from the transform of the new layer -- its margins are parameters, so that too small a rectangle or too short a reach can be
shown to differ from the transform run from scratch.  tests/test_scan_reference.py holds the model equal to
cost_separable(apply_scan(...)) in every bit.  `wrong` names a deliberately wrong version, for that test.
"""
import numpy as np

import costmap_reference as CR

MAX_REACH = 4096   # CCV_MPPI_SCAN_MAX_REACH


def _axes(s, e, wrong=None):
    dx, dy = int(e[0]) - int(s[0]), int(e[1]) - int(s[1])
    adx, ady = abs(dx), abs(dy)
    xmajor = adx > ady if wrong == "ties_to_y" else adx >= ady
    a, b = (adx, ady) if xmajor else (ady, adx)
    assert a <= MAX_REACH
    return xmajor, a, b, (1 if dx >= 0 else -1), (1 if dy >= 0 else -1)


def _place(s, xmajor, major, minor, sgx, sgy):
    x = s[0] + sgx * (major if xmajor else minor)
    y = s[1] + sgy * (minor if xmajor else major)
    return np.stack([x, y], axis=-1).astype(np.int64).reshape(-1, 2)


def ray_cells(s, e, wrong=None):
    """int64 [a][2]: the cells (x, y) of the ray from the sensor cell s to the end cell e, by the closed form"""
    xmajor, a, b, sgx, sgy = _axes(s, e, wrong)
    i = np.arange(a, dtype=np.int64)
    minor = (2 * i * b + (0 if wrong == "no_rounding" else a)) // max(2 * a, 1)
    return _place(s, xmajor, i, minor, sgx, sgy)


def ray_cells_walk(s, e):
    """the same cells by the integer error walk: e = a; per step e += 2b; if e >= 2a: e -= 2a, minor += 1"""
    xmajor, a, b, sgx, sgy = _axes(s, e)
    major, minor, err, m = [], [], a, 0
    for i in range(a):
        major.append(i)
        minor.append(m)
        err += 2 * b
        if err >= 2 * a:
            err -= 2 * a
            m += 1
    return _place(s, xmajor, np.array(major, dtype=np.int64), np.array(minor, dtype=np.int64), sgx, sgy)


def _put(new, xy, value, wrap=False, clamp=False):
    ny, nx = new.shape
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    if wrap:
        x, y = x % nx, y % ny
    if clamp:
        x, y = np.clip(x, 0, nx - 1), np.clip(y, 0, ny - 1)
    inside = (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
    new[y[inside], x[inside]] = value


def apply_scan(cells, sensor, ends, hits, clear=0, mark=255, wrong=None):
    """the layer after one entry: every ray's cells cleared, then the hits' end cells marked; cells outside the map skipped"""
    cells = np.asarray(cells)
    assert cells.dtype == np.uint8 and cells.ndim == 2
    ny, nx = cells.shape
    assert 0 <= sensor[0] < nx and 0 <= sensor[1] < ny
    ends = np.asarray(ends, dtype=np.int64).reshape(-1, 2)
    hits = np.asarray(hits).reshape(-1) != 0
    assert len(ends) == len(hits)
    rays = [ray_cells(sensor, e, wrong) for e in ends]
    if wrong == "end_cleared":
        rays += [ends[[k]] for k in range(len(ends)) if tuple(ends[k]) != tuple(sensor)]
    if wrong == "sensor_not_cleared":
        rays = [r[1:] for r in rays]
    clears = np.concatenate(rays + [np.zeros((0, 2), dtype=np.int64)])
    new = cells.copy()
    if wrong == "marks_first":
        _put(new, ends[hits], mark)
    _put(new, clears, clear, wrap=wrong == "wrapped")
    if wrong != "marks_first":
        _put(new, ends[hits], mark, clamp=wrong == "marks_clamped")
    return new


def scan_box(nx, ny, sensor, ends, with_sensor=True):
    """(x0, y0, w, h): the bounding box of the sensor cell and all end cells, clipped to the map (every cell a ray touches lies in
    the box of its two ends)"""
    pts = np.asarray(ends, dtype=np.int64).reshape(-1, 2)
    if with_sensor or len(pts) == 0:
        pts = np.concatenate([pts, np.asarray(sensor, dtype=np.int64).reshape(1, 2)])
    x0, y0 = max(int(pts[:, 0].min()), 0), max(int(pts[:, 1].min()), 0)
    x1, y1 = min(int(pts[:, 0].max()) + 1, nx), min(int(pts[:, 1].max()) + 1, ny)
    return x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)


def scan_rect(nx, ny, sensor, ends, R, grow=None, with_sensor=True):
    """the rectangle of float cells the entry derives again: scan_box grown by `grow` (default R) and clipped again"""
    box = scan_box(nx, ny, sensor, ends, with_sensor)
    if box[2] == 0 or box[3] == 0:
        return box
    return CR.dilated_rect(box, R if grow is None else grow, nx, ny)


def scan_cost(cost_old, layer_new, sensor, ends, threshold, R, profile, free_value, grow=None, reach=None, with_sensor=True):
    """The scan path as a model: cost_old with scan_rect derived again from layer_new (the layer after the scan), looking only
    at occupancy within `reach` (default 2R) of the box; every other cell kept.  With the defaults this equals the transform
    from scratch on layer_new."""
    ny, nx = layer_new.shape
    box = scan_box(nx, ny, sensor, ends, with_sensor)
    if box[2] == 0 or box[3] == 0:
        return np.array(cost_old, dtype=np.float32, copy=True)
    return CR.patch_cost(cost_old, layer_new, box, threshold, R, profile, free_value, dilate=R if grow is None else grow, reach=reach)


# ---- the cases of the CPU test and of the GPU test -------------------------------------------------------------------------------
def fan(sensor, n, length, hit_every=2, phase=0.0):
    """(ends int64 [n][2], hits uint8 [n]): n rays of `length` cells all round the sensor cell, every hit_every-th one a hit
    (0: none)"""
    t = phase + 2.0 * np.pi * np.arange(n) / n
    ends = np.stack([sensor[0] + np.rint(length * np.cos(t)), sensor[1] + np.rint(length * np.sin(t))], axis=1).astype(np.int64)
    hits = (np.arange(n) % hit_every == 0) if hit_every else np.zeros(n, dtype=bool)
    return ends, hits.astype(np.uint8)


def scans(nx, ny):
    """[(name, sensor, ends, hits)]: a 360-ray fan from the centre, the sensor in each corner, end cells outside on every side,
    zero-length rays, all misses, all rays to one end, and a hit whose end lies on another ray's path in both ray orders"""
    c = (nx // 2, ny // 2)
    out = [("fan", c, *fan(c, 360, 0.45 * max(nx, ny) + 2))]
    for k, s in enumerate(((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1))):
        out.append(("corner_%d" % k, s, *fan(s, 90, 0.7 * max(nx, ny) + 3, hit_every=3, phase=0.1 * k)))
    outside = np.array([(-5, c[1]), (nx + 4, c[1] + 1), (c[0], -5), (c[0] - 1, ny + 4), (-3, -2), (nx + 2, ny + 7), (-1, ny), (nx, -1)], dtype=np.int64)
    out.append(("outside", c, outside, np.ones(len(outside), dtype=np.uint8)))
    out.append(("zero_length", c, np.array([c, c, (c[0] + 1, c[1])], dtype=np.int64), np.array([0, 1, 1], dtype=np.uint8)))
    out.append(("all_misses", c, *fan(c, 120, 0.3 * max(nx, ny) + 2, hit_every=0)))
    one = (min(nx - 1, c[0] + 7), max(0, c[1] - 3))
    out.append(("one_end", c, np.array([one] * 50, dtype=np.int64), (np.arange(50) % 7 == 3).astype(np.uint8)))
    # a long ray and a hit that ends on its path
    far = (c[0] + 24, c[1] + 9) if nx >= ny else (c[0] + 9, c[1] + 24)
    path = ray_cells(c, far)
    on = tuple(int(v) for v in path[len(path) // 2])
    pair = np.array([far, on], dtype=np.int64)
    out.append(("hit_on_path", c, pair, np.array([0, 1], dtype=np.uint8)))
    out.append(("hit_on_path_reversed", c, pair[::-1].copy(), np.array([1, 0], dtype=np.uint8)))
    return out


def layers(nx, ny):
    """(name, cells, threshold): all occupied, 50 % and 2 % random, all free (a scan clears, so most layers start occupied)"""
    return [l for l in CR.layers(nx, ny) if l[0] in ("full", "random_0.5", "random_0.02", "free")]

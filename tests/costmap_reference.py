"""Costmaps inflated on the device (ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue), restated.

The spec, integers and one table lookup:

    occ(ix, iy)  = cells_u8[iy][ix] >= threshold                 a cell outside the map is not occupied
    D2(ix, iy)   = min over occupied (jx, jy) of (jx - ix)^2 + (jy - iy)^2     +inf if there is none
    cost(ix, iy) = profile[D2] if D2 <= R * R else free_value    float32

Two independent restatements: `cost_brute` walks the (2R + 1)^2 window offset by offset with explicit bounds (slices, no
np.roll: nothing wraps), `cost_separable` is the two-pass form in integers (nearest occupied cell of the row by running
maxima from either side, then the minimum over the column of g^2 + dy^2).  tests/test_costmap_reference.py holds them equal
in every bit and shows that each of a list of wrong versions differs somewhere.  `patch_cost` is the patch path as a
model: the rectangle derived again and the occupancy it may look at are parameters, so that too small a rectangle or too short
a reach can be shown to differ from the transform run from scratch.
"""
import numpy as np

FAR = np.iinfo(np.int32).max   # "no occupied cell"


def occupied(cells, threshold):
    cells = np.asarray(cells)
    assert cells.dtype == np.uint8 and cells.ndim == 2
    return cells >= int(threshold)


def window_min(occ, W, dist):
    """min over the offsets |dx|, |dy| <= W whose cell (ix + dx, iy + dy) lies in the map and is occupied of dist(dx, dy), FAR where
    there is none; int64 [ny][nx]"""
    ny, nx = occ.shape
    D = np.full((ny, nx), FAR, dtype=np.int64)
    for dy in range(-W, W + 1):
        if abs(dy) >= ny:
            continue   # (no cell of the map has a cell of the map dy rows away)
        ys = slice(max(0, -dy), min(ny, ny - dy))
        yt = slice(ys.start + dy, ys.stop + dy)
        for dx in range(-W, W + 1):
            if abs(dx) >= nx:
                continue
            xs = slice(max(0, -dx), min(nx, nx - dx))
            xt = slice(xs.start + dx, xs.stop + dx)
            D[ys, xs] = np.where(occ[yt, xt], np.minimum(D[ys, xs], dist(dx, dy)), D[ys, xs])
    return D


def lookup(D2, R, profile, free_value):
    profile = np.asarray(profile, dtype=np.float32)
    assert profile.shape == (R * R + 1,)
    near = D2 <= R * R
    return np.where(near, profile[np.where(near, D2, 0)], np.float32(free_value)).astype(np.float32)


def d2_brute(occ, R):
    return window_min(occ, R, lambda dx, dy: dx * dx + dy * dy)


def cost_brute(cells, threshold, R, profile, free_value):
    return lookup(d2_brute(occupied(cells, threshold), R), R, profile, free_value)


def row_distance(occ, R):
    """g [ny][nx]: the distance to the nearest occupied cell of the same row within +-R, FAR where there is none"""
    ny, nx = occ.shape
    x = np.arange(nx, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(occ, x, -FAR), axis=1)                        # the last occupied column <= x
    right = np.minimum.accumulate(np.where(occ, x, FAR)[:, ::-1], axis=1)[:, ::-1]      # the first occupied column >= x
    g = np.minimum(x - left, right - x)
    return np.where(g <= R, g, FAR)


def d2_separable(occ, R):
    ny, nx = occ.shape
    g = row_distance(occ, R)
    g2 = np.where(g == FAR, FAR, g * g)
    D = np.full((ny, nx), FAR, dtype=np.int64)
    for dy in range(-R, R + 1):
        if abs(dy) >= ny:
            continue
        ys = slice(max(0, -dy), min(ny, ny - dy))
        yt = slice(ys.start + dy, ys.stop + dy)
        D[ys] = np.minimum(D[ys], np.where(g2[yt] == FAR, FAR, g2[yt] + dy * dy))
    return D


def cost_separable(cells, threshold, R, profile, free_value):
    return lookup(d2_separable(occupied(cells, threshold), R), R, profile, free_value)


# ---- patches ---------------------------------------------------------------------------------------------------------------
def apply_patch(cells, x0, y0, patch):
    """a copy of cells [ny][nx] with [y0 : y0 + h, x0 : x0 + w] replaced by patch [h][w]"""
    patch = np.asarray(patch, dtype=np.uint8)
    h, w = patch.shape
    ny, nx = cells.shape
    assert w >= 1 and h >= 1 and 0 <= x0 and x0 + w <= nx and 0 <= y0 and y0 + h <= ny
    out = cells.copy()
    out[y0:y0 + h, x0:x0 + w] = patch
    return out


def dilated_rect(rect, R, nx, ny):
    """(x0, y0, w, h) grown by R cells on every side, clipped to the map"""
    x0, y0, w, h = rect
    ax, ay = max(0, x0 - R), max(0, y0 - R)
    bx, by = min(nx, x0 + w + R), min(ny, y0 + h + R)
    return ax, ay, bx - ax, by - ay


def patch_cost(cost_old, cells_new, rect, threshold, R, profile, free_value, dilate=None, reach=None):
    """The patch path as a model: cost_old with the rectangle `rect` grown by `dilate` (default R) derived again from cells_new (the
    layer after the patch), looking only at occupancy within `reach` (default 2R) of the patch -- every cell further away counts
    as free.  With the defaults this equals the transform from scratch on cells_new."""
    ny, nx = cells_new.shape
    dilate = R if dilate is None else dilate
    reach = 2 * R if reach is None else reach
    ax, ay, aw, ah = dilated_rect(rect, reach, nx, ny)
    seen = np.zeros_like(occupied(cells_new, threshold))
    seen[ay:ay + ah, ax:ax + aw] = occupied(cells_new, threshold)[ay:ay + ah, ax:ax + aw]
    fresh = lookup(d2_separable(seen, R), R, profile, free_value)
    rx, ry, rw, rh = dilated_rect(rect, max(dilate, 0), nx, ny)
    out = np.array(cost_old, dtype=np.float32, copy=True)
    out[ry:ry + rh, rx:rx + rw] = fresh[ry:ry + rh, rx:rx + rw]
    return out


# ---- the cases of the CPU test and of the GPU test's full inflation -----------------------------------------------------------
SHAPES = ((1, 1), (1, 200), (200, 1), (67, 45), (130, 70))   # nx x ny
RADII = (0, 1, 3, 17, 64)
FREE_VALUE, OUTSIDE = -7.0, -3.5


def distinct_profile(R):
    """every entry distinct, none equal to FREE_VALUE or OUTSIDE"""
    return (1000.0 + np.arange(R * R + 1)).astype(np.float32)


def layers(nx, ny, seed=0):
    """[(name, cells uint8 [ny][nx], threshold)]: all free, all occupied, single cells at each corner and the middle of each edge,
    random occupancy at 2 % and 50 %, and random values under the thresholds 0 (everything occupied), 1 and 255"""
    rng = np.random.default_rng(1000 * nx + ny + seed)
    out = [("free", np.zeros((ny, nx), dtype=np.uint8), 100), ("full", np.full((ny, nx), 100, dtype=np.uint8), 100)]
    spots = {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, 0), (nx // 2, ny - 1), (0, ny // 2), (nx - 1, ny // 2)}
    for ix, iy in sorted(spots):
        cells = np.full((ny, nx), 99, dtype=np.uint8)   # (one below the threshold)
        cells[iy, ix] = 100
        out.append(("single_%d_%d" % (ix, iy), cells, 100))
    for share in (0.02, 0.5):
        out.append(("random_%g" % share, np.where(rng.random((ny, nx)) < share, 200, 50).astype(np.uint8), 128))
    values = rng.integers(0, 256, size=(ny, nx)).astype(np.uint8)
    for threshold in (0, 1, 255):
        out.append(("threshold_%d" % threshold, values, threshold))
    return out

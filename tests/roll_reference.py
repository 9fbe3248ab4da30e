"""Rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue), restated on top of costmap_reference.py.

The spec, integers plus one product and one sum per origin: a roll of a map by (dx, dy) cells gives

    new(ix, iy) = old(ix + dx, iy + dy)      where (ix + dx, iy + dy) lies inside the map
                = the caller's cell, or fill elsewhere (the exposed cells)
    origin      = origin0 + (double)c * resolution, c the cells moved since the map was set (never a running sum)
    cost        = the transform of costmap_reference.py over `new`, complete

`roll_layer` is the first line, `pack_strips` / `unpack_strips` the layout of the caller's exposed cells (per entry the row strip,
then the column strip over the remaining rows), `rolled_origin` the third.  `roll_cost` is the band path as a model: the old
cost shifted, and only the bands of `roll_bands` derived again -- their margins are parameters, so that too narrow a band can be
shown to differ from the transform run from scratch.  tests/test_roll_reference.py holds the model equal to
cost_separable(roll_layer(...)) in every bit.
"""
import numpy as np

import costmap_reference as CR


def _spans(n, d):
    """(destination slice, source slice) of the cells of an axis of n cells that stay under a shift by d"""
    lo, hi = max(0, -d), min(n, n - d)
    if hi <= lo:
        return slice(0, 0), slice(0, 0)
    return slice(lo, hi), slice(lo + d, hi + d)


def exposed_mask(nx, ny, dx, dy):
    """bool [ny][nx]: the cells of the new frame whose source (ix + dx, iy + dy) lies outside the map"""
    m = np.ones((ny, nx), dtype=bool)
    (yd, _), (xd, _) = _spans(ny, dy), _spans(nx, dx)
    m[yd, xd] = False
    return m


def strip_rows(ny, dy):
    """(the exposed rows, the remaining rows) of the new frame, each ascending"""
    ay = min(abs(dy), ny)
    rows = np.arange(ny - ay, ny) if dy > 0 else np.arange(0, ay)
    return rows, np.setdiff1d(np.arange(ny), rows)


def strip_cols(nx, dx):
    ax = min(abs(dx), nx)
    return np.arange(nx - ax, nx) if dx > 0 else np.arange(0, ax)


def strips_of(window, dx, dy):
    """the (row strip, column strip) a caller cuts out of its new window [ny][nx] for a roll by (dx, dy)"""
    ny, nx = window.shape
    rows, rest = strip_rows(ny, dy)
    return window[rows, :].copy(), window[np.ix_(rest, strip_cols(nx, dx))].copy()


def roll_layer(cells, dx, dy, strips=None, fill=0):
    """the layer after a roll by (dx, dy): the cells that stay, and the exposed ones from strips = (row strip, column strip) or
    `fill`"""
    cells = np.asarray(cells)
    assert cells.dtype == np.uint8 and cells.ndim == 2
    ny, nx = cells.shape
    new = np.full((ny, nx), fill, dtype=np.uint8)
    if strips is not None:
        rows, rest = strip_rows(ny, dy)
        row_strip, col_strip = strips
        cols = strip_cols(nx, dx)
        assert np.shape(row_strip) == (len(rows), nx) and np.shape(col_strip) == (len(rest), len(cols))
        new[rows, :] = row_strip
        new[np.ix_(rest, cols)] = col_strip
    (yd, ys), (xd, xs) = _spans(ny, dy), _spans(nx, dx)
    new[yd, xd] = cells[ys, xs]
    return new


def pack_strips(entries):
    """the exposed buffer of a call: entry after entry, the row strip and then the column strip, tightly packed"""
    parts = [np.asarray(s, dtype=np.uint8).reshape(-1) for rows, cols in entries for s in (rows, cols)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def unpack_strips(buf, sizes, shifts):
    """the inverse of pack_strips: sizes [(nx, ny)], shifts [(dx, dy)] -> [(row strip, column strip)]"""
    out, at = [], 0
    for (nx, ny), (dx, dy) in zip(sizes, shifts):
        ax, ay = min(abs(dx), nx), min(abs(dy), ny)
        rows = buf[at:at + ay * nx].reshape(ay, nx)
        at += ay * nx
        cols = buf[at:at + (ny - ay) * ax].reshape(ny - ay, ax)
        at += (ny - ay) * ax
        out.append((rows, cols))
    assert at == len(buf)
    return out


def rolled_origin(origin0, c, resolution):
    """the origin after c = (cx, cy) cells: one product and one sum per axis in binary64 (Python floats: no FMA)"""
    return (float(origin0[0]) + float(int(c[0])) * float(resolution), float(origin0[1]) + float(int(c[1])) * float(resolution))


def roll_bands(nx, ny, dx, dy, R, lead=None, trail=None):
    """the rectangles (x0, y0, w, h) whose float cells a roll derives again, clipped to the map: per axis a leading band of
    |d| + lead cells on the side the exposed cells appear and a trailing band of `trail` cells on the side cells left (lead and
    trail default to R); none for an axis that does not move.  They may overlap."""
    lead = R if lead is None else lead
    trail = R if trail is None else trail
    out = []
    for axis, (n, d) in enumerate(((nx, dx), (ny, dy))):
        if d == 0:
            continue
        wl, wt = min(abs(d) + lead, n), min(trail, n)
        for lo, w in ((n - wl, wl), (0, wt)) if d > 0 else ((0, wl), (n - wt, wt)):
            if w > 0:
                out.append((lo, 0, w, ny) if axis == 0 else (0, lo, nx, w))
    return out


def roll_cost(cost_old, layer_new, dx, dy, threshold, R, profile, free_value, lead=None, trail=None):
    """The band path as a model: cost_old shifted by (dx, dy), then the bands derived again from layer_new (the complete layer
    after the roll).  A cell that neither the shift nor a band writes is NaN.  With the default margins this equals the
    transform from scratch on layer_new."""
    ny, nx = layer_new.shape
    out = np.full((ny, nx), np.nan, dtype=np.float32)
    (yd, ys), (xd, xs) = _spans(ny, dy), _spans(nx, dx)
    out[yd, xd] = np.asarray(cost_old, dtype=np.float32)[ys, xs]
    fresh = CR.cost_separable(layer_new, threshold, R, profile, free_value)
    for x0, y0, w, h in roll_bands(nx, ny, dx, dy, R, lead, trail):
        out[y0:y0 + h, x0:x0 + w] = fresh[y0:y0 + h, x0:x0 + w]
    return out


# ---- the cases of the CPU test and of the GPU test --------------------------------------------------------------------------------
def shifts(nx, ny):
    """the fixed shifts, the ones that expose all but one column, every column, and everything in both axes; each with both signs
    flipped as well"""
    base = [(0, 0), (1, 0), (0, -1), (3, -2), (-64, 5), (nx - 1, 0), (nx, 0), (nx + 5, -ny)]
    out = []
    for s in base + [(-dx, -dy) for dx, dy in base]:
        if s not in out:
            out.append(s)
    return out


def layers(nx, ny):
    """(name, cells, threshold): all free, all occupied, a single occupied cell on each edge and corner (the cell that leaves the
    map), 2 % and 50 % random"""
    return [l for l in CR.layers(nx, ny) if not l[0].startswith("threshold_")]

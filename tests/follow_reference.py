"""Costmaps that follow their robots (ccv_mppi_batch_resident_follow_enqueue), restated.

The spec.  For a map with nx x ny cells, resolution, the origin it was set with (origin0), its frame as the call finds it
(cx, cy, origin_x, origin_y) and the pose (x, y) of the robot on it:

    fx = (x - origin_x) * inv,  fy likewise     (inv = RN(1 / resolution); one subtraction, one multiplication, no FMA)
    ok = fabs(fx) < 2^30 && fabs(fy) < 2^30     (false for a NaN or infinite pose)
    px = (int64)floor(fx), py likewise          (floor, not truncation: the pose may lie left of or below the map)
    ex = px - nx / 2,  ey = py - ny / 2         (C integer division: the centre cell)
    dx = |ex| <= margin ? 0 : clamp(ex, -max_step, max_step)      dy likewise, each axis on its own
    cx' = cx + dx, cy' = cy + dy;  |cx'| > 2^30 or |cy'| > 2^30, or a rolled origin not finite: nothing moves
    origin' = origin0 + (double)cx' * resolution    (one multiplication, one addition, no FMA: the host roll's formula)
    status: 1 MOVED, 2 HELD (dx = dy = 0), 3 NO_POSE (!ok), 4 LIMIT; 0: the map has never been followed

On MOVED the map is rolled by (dx, dy) with every exposed cell `fill` (roll_reference.roll_layer); on every other status nothing
changes.  Python floats are IEEE doubles and Python evaluates a * b + c in two roundings, so `decide` is the statement above as it
stands.  `wrong=` names one of MUTATIONS, a plausible other reading of the spec; tests/test_follow_reference.py shows that each
differs from the spec on a listed case.  `rolled_origin_exact` is the origin formula in rational arithmetic, rounded once per
operation.  `bands` restates roll_bands (csrc/mppi_costmap_rects.h), the one statement of the band arithmetic the host's rolls
and the device's follows share.
"""
import math
from fractions import Fraction

MOVED, HELD, NO_POSE, LIMIT = 1, 2, 3, 4
LIMIT_CELLS = 2 ** 30
MUTATIONS = ("trunc", "lt_margin", "no_clamp", "centre", "origin_sum", "coupled")


def _clamp(e, m):
    return max(-m, min(m, e))


def decide(frame, pose, geometry, margin, max_step, wrong=None):
    """(status, dx, dy, frame') for frame = (cx, cy, origin_x, origin_y), pose = (x, y), geometry = ((origin0_x, origin0_y),
    resolution, nx, ny)"""
    assert wrong is None or wrong in MUTATIONS, wrong
    cx, cy, ox, oy = frame
    (ox0, oy0), resolution, nx, ny = geometry
    inv = 1.0 / resolution
    fx, fy = (pose[0] - ox) * inv, (pose[1] - oy) * inv
    if not (abs(fx) < 2.0 ** 30 and abs(fy) < 2.0 ** 30):   # (a NaN compares false)
        return NO_POSE, 0, 0, frame
    cell = math.trunc if wrong == "trunc" else math.floor
    centre = (lambda n: (n - 1) // 2) if wrong == "centre" else (lambda n: n // 2)
    ex, ey = cell(fx) - centre(nx), cell(fy) - centre(ny)
    inside = (lambda e: abs(e) < margin) if wrong == "lt_margin" else (lambda e: abs(e) <= margin)
    step = (lambda e: e) if wrong == "no_clamp" else (lambda e: _clamp(e, max_step))
    if wrong == "coupled":
        still = inside(ex) and inside(ey)
        dx, dy = (0, 0) if still else (step(ex), step(ey))
    else:
        dx, dy = 0 if inside(ex) else step(ex), 0 if inside(ey) else step(ey)
    if dx == 0 and dy == 0:
        return HELD, 0, 0, frame
    ncx, ncy = cx + dx, cy + dy
    if abs(ncx) > LIMIT_CELLS or abs(ncy) > LIMIT_CELLS:
        return LIMIT, 0, 0, frame
    if wrong == "origin_sum":
        nox, noy = ox + float(dx) * resolution, oy + float(dy) * resolution
    else:
        nox, noy = ox0 + float(ncx) * resolution, oy0 + float(ncy) * resolution
    if not (math.isfinite(nox) and math.isfinite(noy)):
        return LIMIT, 0, 0, frame
    return MOVED, dx, dy, (ncx, ncy, nox, noy)


def _rn(q):
    """the double nearest the rational q (ties to even): float(Fraction) rounds correctly"""
    return float(q)


def rolled_origin_exact(origin0, c, resolution):
    """origin0 + (double)c * resolution with each of the two operations rounded once, in rational arithmetic"""
    product = _rn(Fraction(float(c)) * Fraction(resolution))
    return _rn(Fraction(origin0) + Fraction(product))


def bands(nx, ny, ex, ey, R):
    """roll_bands of csrc/mppi_costmap_rects.h: the non-empty ones of the four rectangles (x0, y0, w, h), in its order"""
    lx = min(abs(ex) + R, nx) if ex else 0
    tx = min(R, nx - lx) if ex else 0
    ly = min(abs(ey) + R, ny) if ey else 0
    ty = min(R, ny - ly) if ey else 0
    xa, xb = (tx, nx - lx) if ex > 0 else (lx, nx - tx)
    out = [(nx - lx if ex > 0 else 0, 0, lx, ny), (0 if ex > 0 else nx - tx, 0, tx, ny),
           (xa, ny - ly if ey > 0 else 0, xb - xa, ly), (xa, 0 if ey > 0 else ny - ty, xb - xa, ty)]
    return [r for r in out if r[2] >= 1 and r[3] >= 1]


def pose_for(frame, geometry, cell, frac=(0.5, 0.5)):
    """a pose in cell `cell` = (ix, iy) of the frame (cells may be negative or beyond the map), `frac` of a cell in; for
    resolutions that are powers of two and origins that are multiples of them the pose is exact and frac = 0 lies on the edge"""
    _, _, ox, oy = frame
    resolution = geometry[1]
    return ox + (cell[0] + frac[0]) * resolution, oy + (cell[1] + frac[1]) * resolution

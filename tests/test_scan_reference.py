"""CPU checks of the scan-tracing restatement (tests/scan_reference.py): the closed form of a ray equals
the integer error walk, a ray is what the spec says cell by cell, the scan path -- the old cost with one rectangle derived again --
equals the transform run from scratch on the scanned layer in every bit, each of a list of wrong versions differs somewhere, and
batch.scan_cells turns ranges into end cells by the rules of its docstring."""
import os
import sys

import numpy as np
import pytest

import costmap_reference as CR
import scan_reference as SR
from ccv_mppi_path_tracker_amd import batch, capi, configs

FREE = CR.FREE_VALUE


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- one ray ----------------------------------------------------------------------------------------------------------------------
def check_ray(s, e):
    cells, a = SR.ray_cells(s, e), max(abs(e[0] - s[0]), abs(e[1] - s[1]))
    assert same(cells, SR.ray_cells_walk(s, e)), (s, e)
    assert len(cells) == a
    if a == 0:
        return
    assert tuple(cells[0]) == tuple(s)
    steps = np.diff(np.concatenate([cells, np.array([e], dtype=np.int64)]), axis=0)   # (stepping once more reaches the end cell)
    assert np.abs(steps).max() == 1 and (np.abs(steps).max(axis=1) == 1).all(), (s, e)


def test_the_closed_form_is_the_error_walk_in_a_square_around_the_sensor():
    s = (7, -3)
    for dy in range(-40, 41):
        for dx in range(-40, 41):
            check_ray(s, (s[0] + dx, s[1] + dy))


@pytest.mark.parametrize("reach", (4095, 4096))
def test_the_closed_form_is_the_error_walk_at_the_longest_reach(reach):
    s = (100, 50)
    assert reach <= SR.MAX_REACH == capi.SCAN_MAX_REACH and 2 * (reach - 1) * reach + reach < 2 ** 26
    for b in (0, 1, 2, reach // 3, reach // 2, reach - 1, reach):   # on the axes, inside every octant, on the diagonals
        for sgx in (-1, 1):
            for sgy in (-1, 1):
                check_ray(s, (s[0] + sgx * reach, s[1] + sgy * b))
                check_ray(s, (s[0] + sgx * b, s[1] + sgy * reach))


def test_a_ray_cell_by_cell():
    """the spec's worked cases: ties go to x, the minor coordinate rounds to nearest with halves up, the end cell stays"""
    assert SR.ray_cells((2, 3), (2, 3)).shape == (0, 2)
    assert SR.ray_cells((0, 0), (4, 0)).tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]
    assert SR.ray_cells((0, 0), (-3, 3)).tolist() == [[0, 0], [-1, 1], [-2, 2]]
    assert SR.ray_cells((0, 0), (4, 2)).tolist() == [[0, 0], [1, 1], [2, 1], [3, 2]]       # (4 i + 4) div 8: the half at i = 1 goes up
    assert SR.ray_cells((0, 0), (2, -4)).tolist() == [[0, 0], [1, -1], [1, -2], [2, -3]]
    assert SR.ray_cells((5, 5), (5, 2)).tolist() == [[5, 5], [5, 4], [5, 3]]


# ---- a scan against the transform from scratch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", CR.RADII)
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_the_scan_path_equals_the_transform_from_scratch(nx, ny, R):
    profile = CR.distinct_profile(R)
    for lname, cells, threshold in SR.layers(nx, ny):
        cost_old = CR.cost_separable(cells, threshold, R, profile, FREE)
        for name, sensor, ends, hits in SR.scans(nx, ny):
            new = SR.apply_scan(cells, sensor, ends, hits, clear=0, mark=255)
            got = SR.scan_cost(cost_old, new, sensor, ends, threshold, R, profile, FREE)
            assert same(got, CR.cost_separable(new, threshold, R, profile, FREE)), (lname, name)
            x0, y0, w, h = SR.scan_rect(nx, ny, sensor, ends, R)
            changed = np.argwhere(new != cells)
            assert w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= nx and y0 + h <= ny
            bx, by, bw, bh = SR.scan_box(nx, ny, sensor, ends)
            assert all(by <= y < by + bh and bx <= x < bx + bw for y, x in changed), (lname, name)


def test_apply_scan_is_the_spec_cell_by_cell():
    nx, ny = 9, 7
    cells = np.full((ny, nx), 100, dtype=np.uint8)
    s = (4, 3)
    ends = np.array([(8, 3), (4, 3), (4, -2), (12, 5), (0, 0)], dtype=np.int64)
    hits = np.array([1, 1, 1, 1, 0], dtype=np.uint8)
    want = cells.copy()
    for e in ends:
        for x, y in SR.ray_cells_walk(s, e):
            if 0 <= x < nx and 0 <= y < ny:
                want[y, x] = 7
    want[3, 8] = want[3, 4] = 200   # (the marks inside the map: the end of ray 0, and the sensor cell as the end of a zero-length hit)
    assert same(SR.apply_scan(cells, s, ends, hits, clear=7, mark=200), want)
    assert want[0, 0] == 100 and want[1, 1] == 7   # (a miss leaves its end cell as it was)
    # an entry without rays, and one of zero-length misses, change nothing
    assert same(SR.apply_scan(cells, s, np.zeros((0, 2)), np.zeros(0)), cells)
    assert same(SR.apply_scan(cells, s, [s, s], [0, 0]), cells)


def test_marks_win_whatever_the_order():
    for nx, ny in ((67, 45), (130, 70)):
        for name, sensor, ends, hits in SR.scans(nx, ny):
            cells = np.full((ny, nx), 100, dtype=np.uint8)
            a = SR.apply_scan(cells, sensor, ends, hits, clear=0, mark=255)
            assert same(a, SR.apply_scan(cells, sensor, ends[::-1], hits[::-1], clear=0, mark=255)), name
    # the two orders of the pair are two inputs with one result
    by_name = {s[0]: s for s in SR.scans(67, 45)}
    p, q = by_name["hit_on_path"], by_name["hit_on_path_reversed"]
    cells = np.full((45, 67), 100, dtype=np.uint8)
    a, b = SR.apply_scan(cells, *p[1:]), SR.apply_scan(cells, *q[1:])
    on = p[2][1]
    assert same(a, b) and a[on[1], on[0]] == 255 and any((SR.ray_cells(p[1], p[2][0]) == on).all(axis=1))


# ---- wrong versions ---------------------------------------------------------------------------------------------------------------
def wrong_case():
    nx, ny = 67, 45
    cells = np.full((ny, nx), 100, dtype=np.uint8)
    scans = {s[0]: s[1:] for s in SR.scans(nx, ny)}
    return nx, ny, cells, scans


@pytest.mark.parametrize("wrong,scan", [("end_cleared", "all_misses"), ("marks_first", "hit_on_path"), ("marks_first", "hit_on_path_reversed"),
                                        ("no_rounding", "fan"), ("sensor_not_cleared", "all_misses"),
                                        ("wrapped", "outside"), ("marks_clamped", "outside")])
def test_wrong_tracings_differ(wrong, scan):
    nx, ny, cells, scans = wrong_case()
    sensor, ends, hits = scans[scan]
    good = SR.apply_scan(cells, sensor, ends, hits, clear=0, mark=255)
    assert not same(SR.apply_scan(cells, sensor, ends, hits, clear=0, mark=255, wrong=wrong), good)


def test_ties_to_the_other_axis_cannot_differ():
    """The one wrong version of the list that is not wrong: on a tie a = b, so the minor offset (2 i a + a) div (2 a) is i, and
    the cells are (s + sign * i, s + sign * i) whichever axis is called the major one.  Held here so that nobody looks for the
    difference again; the rule `x if adx >= ady` still fixes which axis the spec's words mean."""
    for d in range(0, 41):
        for sgx in (-1, 1):
            for sgy in (-1, 1):
                e = (3 + sgx * d, -2 + sgy * d)
                assert same(SR.ray_cells((3, -2), e, wrong="ties_to_y"), SR.ray_cells((3, -2), e))
    assert not same(SR.ray_cells((0, 0), (4, 2), wrong="no_rounding"), SR.ray_cells((0, 0), (4, 2)))


@pytest.mark.parametrize("R", (3, 17))
def test_wrong_rectangles_differ(R):
    """a scan that clears a block which stood R cells inside the rays' box edge, and marks a cell on the edge: the cost changes up
    to R beyond the box, and the occupancy that takes over lies up to 2R from it"""
    nx, ny = 130, 120
    profile = CR.distinct_profile(R)
    s = (40, 40)
    ends = np.array([(100, 40), (100, 41), (70, 40 - R - 5)], dtype=np.int64)
    hits = np.array([1, 0, 0], dtype=np.uint8)
    cells = np.zeros((ny, nx), dtype=np.uint8)
    cells[40, 50:95] = 1                  # cleared by the first ray
    cells[41 + 2 * R, 60] = 1             # 2R beyond the box's edge y = 41: the cells R beyond that edge take their cost from it
    cells[40, s[0] - 2 * R] = 1           # 2R left of the sensor cell, the box's left edge
    cost_old = CR.cost_separable(cells, 1, R, profile, FREE)
    new = SR.apply_scan(cells, s, ends, hits, clear=0, mark=1)
    want = CR.cost_separable(new, 1, R, profile, FREE)
    assert not same(want, cost_old)
    assert same(SR.scan_cost(cost_old, new, s, ends, 1, R, profile, FREE), want)
    for margins in (dict(grow=0), dict(grow=R - 1), dict(reach=R), dict(reach=2 * R - 1)):
        assert not same(SR.scan_cost(cost_old, new, s, ends, 1, R, profile, FREE, **margins), want), margins
    # (and one cell more than needed changes nothing)
    assert same(SR.scan_cost(cost_old, new, s, ends, 1, R, profile, FREE, grow=R + 1, reach=2 * R + 1), want)
    # the rectangle without the sensor cell: the first cells of every ray are cleared outside it
    cells2 = np.ones((ny, nx), dtype=np.uint8)
    ends2 = np.array([(90, 35), (90, 50)], dtype=np.int64)
    old2 = CR.cost_separable(cells2, 1, R, profile, FREE)
    new2 = SR.apply_scan(cells2, (2, 2), ends2, [0, 0], clear=0, mark=1)
    want2 = CR.cost_separable(new2, 1, R, profile, FREE)
    assert same(SR.scan_cost(old2, new2, (2, 2), ends2, 1, R, profile, FREE), want2)
    assert not same(SR.scan_cost(old2, new2, (2, 2), ends2, 1, R, profile, FREE, with_sensor=False), want2)


# ---- batch.scan_cells -----------------------------------------------------------------------------------------------------------------
GEO = ((-1.7, 0.3), 0.05, 0.0, 200, 160, 128, 6, 0.0)   # an entry of BatchController.get_occupancy()


def test_scan_cells_puts_every_kept_point_in_its_cell():
    (ox, oy), res = GEO[0], GEO[1]
    pos, yaw = (2.31, 3.77), 0.4
    n = 360
    rng = np.random.default_rng(3)
    ranges = rng.uniform(0.2, 9.0, n)
    ranges[[5, 17]] = np.nan
    ranges[[6, 40]] = 0.05          # below range_min
    ranges[[7, 50]] = [np.inf, 12.5]   # at or past range_max
    ranges[8] = -np.inf
    amin, ainc, rmin, rmax = -np.pi, 2 * np.pi / n, 0.1, 10.0
    (sx, sy), ends, hits = batch.scan_cells(GEO, pos, yaw, ranges, amin, ainc, rmin, rmax)
    kept = [k for k in range(n) if k not in (5, 17, 6, 40, 8)]
    assert ends.dtype == np.int32 and hits.dtype == np.uint8 and ends.shape == (len(kept), 2) and hits.shape == (len(kept),)
    assert (sx, sy) == (int(np.floor((pos[0] - ox) / res)), int(np.floor((pos[1] - oy) / res)))
    inv = 1.0 / res
    for j, k in enumerate(kept):
        r = min(ranges[k], rmax)
        px, py = pos[0] + r * np.cos(yaw + amin + k * ainc), pos[1] + r * np.sin(yaw + amin + k * ainc)
        fx, fy = (px - ox) * inv, (py - oy) * inv
        assert ends[j, 0] <= fx < ends[j, 0] + 1 and ends[j, 1] <= fy < ends[j, 1] + 1, k
        assert hits[j] == (0 if k in (7, 50) else 1), k
    # a point left of and below the origin gets negative cells, not cells truncated towards zero
    (sx, sy), ends, hits = batch.scan_cells(GEO, (-1.68, 0.32), 0.0, [0.5, 0.5], np.pi, 0.5 * np.pi, 0.1, 10.0)
    assert (sx, sy) == (0, 0) and ends.tolist() == [[-10, 0], [0, -10]] and hits.tolist() == [1, 1]
    (sx, sy), ends, _ = batch.scan_cells(GEO, (-1.71, 0.29), 0.0, [0.03], np.pi, 0.0, 0.0, 10.0)
    assert (sx, sy) == (-1, -1) and ends.tolist() == [[-1, -1]]
    # no beam left
    _, ends, hits = batch.scan_cells(GEO, pos, yaw, [np.nan, 0.0], 0.0, 0.1, 0.1, 10.0)
    assert ends.shape == (0, 2) and hits.shape == (0,) and ends.dtype == np.int32


def test_scan_cells_cuts_a_ray_beyond_the_reach_along_itself():
    geo = ((0.0, 0.0), 0.01) + GEO[2:]
    pos = (0.005, 0.005)
    for ang in (0.0, 0.3, np.pi / 4, 2.0, -2.7, np.pi):
        (sx, sy), ends, hits = batch.scan_cells(geo, pos, 0.0, [60.0, 30.0], ang, 0.0, 0.1, 100.0)
        full = (int(np.floor((pos[0] + 60.0 * np.cos(ang)) * (1.0 / 0.01))), int(np.floor((pos[1] + 60.0 * np.sin(ang)) * (1.0 / 0.01))))
        a = max(abs(full[0] - sx), abs(full[1] - sy))
        assert a > capi.SCAN_MAX_REACH
        xmajor = abs(full[0] - sx) >= abs(full[1] - sy)
        b = min(abs(full[0] - sx), abs(full[1] - sy))
        minor = (2 * capi.SCAN_MAX_REACH * b + a) // (2 * a)
        sgx, sgy = (1 if full[0] >= sx else -1), (1 if full[1] >= sy else -1)
        cut = (sx + sgx * (capi.SCAN_MAX_REACH if xmajor else minor), sy + sgy * (minor if xmajor else capi.SCAN_MAX_REACH))
        assert tuple(ends[0]) == cut and hits[0] == 0, ang
        assert max(abs(ends[0, 0] - sx), abs(ends[0, 1] - sy)) == capi.SCAN_MAX_REACH
        # the ray cut is the beginning of the ray whole: the same cells cleared (the closed form with the uncut a and b)
        i = np.arange(capi.SCAN_MAX_REACH, dtype=np.int64)
        whole_minor = (2 * i * b + a) // (2 * a)
        whole = np.stack([sx + sgx * np.where(xmajor, i, whole_minor), sy + sgy * np.where(xmajor, whole_minor, i)], axis=1)
        got = SR.ray_cells((sx, sy), ends[0])
        assert np.abs(got - whole).max() <= 1
        # the second beam, 3000 cells, stays a hit in its own cell
        assert hits[1] == 1 and max(abs(ends[1, 0] - sx), abs(ends[1, 1] - sy)) <= 3001


# ---- the obstacle scene of tests/test_gpu_batch_scan.py, on the door's CPU restatement ------------------------------------------------
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import costmap_door_cpu as CD  # noqa: E402
from costmap_support import CLEAR_TICK, block_scans  # noqa: E402


def test_the_obstacle_scene_on_the_doors_cpu_restatement():
    """the marking scan gives the door's layer (test_costmap_door_cpu.py: no pose in the block's cells with it, some without), every
    ray of both scans is within the reach, and by CLEAR_TICK the robot that saw the block is more than a cell from the one that did
    not: the clearing scan comes when the block has mattered"""
    s, marking, clearing = block_scans()
    assert 0 <= s[0] < CD.NX and 0 <= s[1] < CD.NY
    for ends in (marking[0], clearing[0]):
        assert np.abs(ends - np.array(s)).max() <= capi.SCAN_MAX_REACH
        assert all((SR.ray_cells(s, e) == c).all(axis=1).any() for e, c in zip(clearing[0][::11], marking[0][::11]))
    p = configs.diff_drive_defaults(CD.SAMPLES, 15)
    assert CD.PATCH_TICK < CLEAR_TICK < CD.TICKS
    off, on = CD.drive(p, CD.WEIGHT, False, ticks=CLEAR_TICK + 1), CD.drive(p, CD.WEIGHT, True, ticks=CLEAR_TICK + 1)
    assert np.hypot(*(off[CLEAR_TICK] - on[CLEAR_TICK])) > CD.RESOLUTION
    assert CD.in_block(on) == 0 and on[CLEAR_TICK, 0] < CD.BLOCK["x0"]   # (still in front of the block)

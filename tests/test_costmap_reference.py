"""CPU checks of tests/costmap_reference.py: the two restatements of the inflation equal in every bit over
the shapes, radii, layers and thresholds the GPU test uses; every wrong version of a list differs from the spec in some case;
the patch path's model equals the transform from scratch and its three short-cuts do not; the hand-painted inflation ring of
tools/grid_wall_cpu.py is what a step profile makes of the bare block.  No GPU."""
import os
import sys

import numpy as np
import pytest

import costmap_reference as CR
from ccv_mppi_path_tracker_amd import batch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import grid_wall_cpu as GW  # noqa: E402


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("R", CR.RADII)
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_the_two_restatements_agree_in_every_bit(nx, ny, R):
    profile = CR.distinct_profile(R)
    assert len(set(profile.tolist())) == R * R + 1 and CR.FREE_VALUE not in profile and CR.OUTSIDE not in profile
    for name, cells, threshold in CR.layers(nx, ny):
        a = CR.cost_brute(cells, threshold, R, profile, CR.FREE_VALUE)
        b = CR.cost_separable(cells, threshold, R, profile, CR.FREE_VALUE)
        assert same_bits(a, b), (name, nx, ny, R)
        occ = CR.occupied(cells, threshold)
        assert np.all(a[occ] == profile[0]) and (occ.any() or np.all(a == np.float32(CR.FREE_VALUE))), (name, nx, ny, R)
        if name == "threshold_0":
            assert occ.all()


def test_known_values():
    """one occupied cell in the middle of 9 x 7, R = 2: the cost of every cell by hand"""
    cells = np.zeros((7, 9), dtype=np.uint8)
    cells[3, 4] = 1
    profile = np.array([10, 11, 12, 13, 14], dtype=np.float32)
    want = np.full((7, 9), -1.0, dtype=np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx * dx + dy * dy <= 4:
                want[3 + dy, 4 + dx] = 10 + dx * dx + dy * dy
    assert same_bits(CR.cost_brute(cells, 1, 2, profile, -1.0), want)
    assert same_bits(CR.cost_separable(cells, 1, 2, profile, -1.0), want)


# ---- wrong versions: each differs from the spec somewhere ------------------------------------------------------------------
def _cost(cells, threshold, R, profile, free, d2):
    return CR.lookup(d2(CR.occupied(cells, threshold)), R, profile, free)


def chebyshev(cells, threshold, R, profile, free):
    return _cost(cells, threshold, R, profile, free, lambda occ: CR.window_min(occ, R, lambda dx, dy: max(abs(dx), abs(dy)) ** 2))


def manhattan(cells, threshold, R, profile, free):
    return _cost(cells, threshold, R, profile, free, lambda occ: CR.window_min(occ, R, lambda dx, dy: (abs(dx) + abs(dy)) ** 2))


def short_window(cells, threshold, R, profile, free):
    return _cost(cells, threshold, R, profile, free, lambda occ: CR.window_min(occ, max(R - 1, 0), lambda dx, dy: dx * dx + dy * dy))


def strict_threshold(cells, threshold, R, profile, free):
    return CR.lookup(CR.d2_brute(cells > threshold, R), R, profile, free)


def index_off_by_one(cells, threshold, R, profile, free):
    D2 = CR.d2_brute(CR.occupied(cells, threshold), R)
    return CR.lookup(np.where(D2 <= R * R, np.maximum(D2 - 1, 0), D2), R, profile, free)


def wrapping(cells, threshold, R, profile, free):
    occ = CR.occupied(cells, threshold)
    D = np.full(occ.shape, CR.FAR, dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            D = np.where(np.roll(occ, (-dy, -dx), axis=(0, 1)), np.minimum(D, dx * dx + dy * dy), D)
    return CR.lookup(D, R, profile, free)


def transposed(cells, threshold, R, profile, free):
    ny, nx = cells.shape
    return CR.cost_brute(np.ascontiguousarray(cells.reshape(nx, ny).T), threshold, R, profile, free)   # (cell (ix, iy) read at [ix * ny + iy])


WRONG = [chebyshev, manhattan, short_window, strict_threshold, index_off_by_one, wrapping, transposed]


@pytest.mark.parametrize("wrong", WRONG, ids=lambda f: f.__name__)
def test_a_wrong_version_differs_from_the_spec(wrong):
    differs = 0
    for nx, ny in ((67, 45), (1, 200)):
        for R in (1, 3):
            profile = CR.distinct_profile(R)
            for name, cells, threshold in CR.layers(nx, ny):
                spec = CR.cost_brute(cells, threshold, R, profile, CR.FREE_VALUE)
                differs += not same_bits(spec, wrong(cells, threshold, R, profile, CR.FREE_VALUE))
    assert differs > 0


# ---- the patch path --------------------------------------------------------------------------------------------------------
def test_dilated_rect_and_apply_patch():
    assert CR.dilated_rect((10, 5, 3, 2), 4, 67, 45) == (6, 1, 11, 10)
    assert CR.dilated_rect((1, 0, 3, 2), 4, 67, 45) == (0, 0, 8, 6)
    assert CR.dilated_rect((60, 40, 7, 5), 4, 67, 45) == (56, 36, 11, 9)
    assert CR.dilated_rect((10, 5, 3, 2), 0, 67, 45) == (10, 5, 3, 2)
    cells = np.zeros((4, 5), dtype=np.uint8)
    out = CR.apply_patch(cells, 1, 2, np.array([[7, 8, 9]], dtype=np.uint8))
    assert not cells.any() and out[2].tolist() == [0, 7, 8, 9, 0] and out.sum() == 24


@pytest.mark.parametrize("R", (0, 1, 3, 17))
def test_the_patch_model_equals_the_transform_from_scratch(R):
    rng = np.random.default_rng(R)
    nx, ny, threshold = 67, 45, 128
    profile = CR.distinct_profile(R)
    cells = np.where(rng.random((ny, nx)) < 0.05, 200, 50).astype(np.uint8)
    cost = CR.cost_separable(cells, threshold, R, profile, CR.FREE_VALUE)
    for i in range(12):
        w, h = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        x0, y0 = int(rng.integers(0, nx - w + 1)), int(rng.integers(0, ny - h + 1))
        patch = np.where(rng.random((h, w)) < (0.0 if i % 3 == 0 else 0.3), 200, 50).astype(np.uint8)   # (every third one only clears)
        cells = CR.apply_patch(cells, x0, y0, patch)
        cost = CR.patch_cost(cost, cells, (x0, y0, w, h), threshold, R, profile, CR.FREE_VALUE)
        assert same_bits(cost, CR.cost_separable(cells, threshold, R, profile, CR.FREE_VALUE)), i


@pytest.mark.parametrize("R", (1, 3, 17))
@pytest.mark.parametrize("short_cut", ["undilated", "dilated_by_R_minus_1", "reach_R"])
def test_a_short_cut_of_the_patch_path_differs(short_cut, R):
    """a 1 x 1 patch clears the occupied cell A; B, 2R to its right, stays.  The cell R to the right of A was R from A and is R
    from B: it keeps profile[R * R], which only a reach of 2R from the patch can see; the cell R to the left of A becomes free,
    which only a rectangle grown by R derives again."""
    nx, ny, threshold = 67, 45, 1
    profile = CR.distinct_profile(R)
    cells = np.zeros((ny, nx), dtype=np.uint8)
    ax, ay = 20, 20
    cells[ay, ax] = cells[ay, ax + 2 * R] = 1
    cost = CR.cost_separable(cells, threshold, R, profile, CR.FREE_VALUE)
    new = CR.apply_patch(cells, ax, ay, np.zeros((1, 1), dtype=np.uint8))
    want = CR.cost_separable(new, threshold, R, profile, CR.FREE_VALUE)
    assert want[ay, ax + R] == profile[R * R] and want[ay, ax - R] == np.float32(CR.FREE_VALUE) and cost[ay, ax - R] == profile[R * R]
    kw = dict(undilated=dict(dilate=0), dilated_by_R_minus_1=dict(dilate=R - 1), reach_R=dict(reach=R))[short_cut]
    assert same_bits(CR.patch_cost(cost, new, (ax, ay, 1, 1), threshold, R, profile, CR.FREE_VALUE), want)
    assert not same_bits(CR.patch_cost(cost, new, (ax, ay, 1, 1), threshold, R, profile, CR.FREE_VALUE, **kw), want)


# ---- inflation_profile, and the hand-painted ring it replaces ----------------------------------------------------------------
def test_inflation_profiles():
    R, prof, free = batch.inflation_profile(0.3, 0.05, kind="linear", lethal=4.0, free_value=1.0)
    assert R == 6 and prof.dtype == np.float32 and prof.shape == (37,) and free == 1.0
    assert prof[0] == 4.0 and prof[36] == np.float32(1.0) and np.all(np.diff(prof) <= 0) and np.isclose(prof[9], 2.5)
    R, prof, free = batch.inflation_profile(0.5, 0.1, kind="exponential", lethal=254.0, inscribed=253.0, inscribed_m=0.2, scaling=3.0)
    assert R == 5 and prof[0] == 254.0 and prof[1] == 253.0 and prof[4] == 253.0 and np.isclose(prof[9], 253.0 * np.exp(-0.3))
    assert np.isclose(prof[25], 253.0 * np.exp(-0.9)) and free == 0.0 and np.all(np.isfinite(prof))
    R, prof, _ = batch.inflation_profile(0.0, 0.05)
    assert R == 0 and prof.tolist() == [1.0]
    R, prof, _ = batch.inflation_profile(64 * 0.05, 0.05)
    assert R == 64 and prof.shape == (4097,)
    for bad in (dict(radius_m=65 * 0.05, resolution=0.05), dict(radius_m=0.1, resolution=0.05, kind="quadratic"),
                dict(radius_m=0.1, resolution=0.05, inscribed_m=0.2), dict(radius_m=0.1, resolution=0.0)):
        with pytest.raises(ValueError):
            batch.inflation_profile(**bad)


def test_a_step_profile_makes_the_wall_tests_ring_from_the_bare_block():
    """tools/grid_wall_cpu.py paints 0.5 on the cells whose centre is within 0.15 m of the block's rectangle: measured between the
    centres of cells that is D2 <= 13 (every offset to the nearest occupied cell up to (3, 2); (4, 0) and (3, 3) are outside),
    a step of 0.185 m at 0.05 m cells."""
    g = GW.wall_map(**GW.WALL)
    bare = (g.cells == 1.0).astype(np.uint8)
    assert 0 < bare.sum() < bare.size
    R, prof, free = batch.inflation_profile(0.185, g.resolution, kind="step", lethal=1.0, inscribed=0.5, free_value=0.0)
    assert R == 4 and prof[13] == 0.5 and prof[14] == 0.0
    for cost in (CR.cost_brute, CR.cost_separable):
        assert same_bits(cost(bare, 1, R, prof, free), g.cells)

"""CPU checks of the rolling-costmap restatement (tests/roll_reference.py): the band path -- the old cost
shifted, four bands derived again -- equals the transform run from scratch on the rolled layer in every bit, and each of a list
of wrong versions differs somewhere."""
import numpy as np
import pytest

import costmap_reference as CR
import roll_reference as RR

FREE = CR.FREE_VALUE


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def window(nx, ny, seed):
    """a caller's new window: random cells around the threshold of the random layers"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((ny, nx)) < 0.1, 200, 50).astype(np.uint8)


@pytest.mark.parametrize("R", CR.RADII)
@pytest.mark.parametrize("nx,ny", CR.SHAPES)
def test_the_band_path_equals_the_transform_from_scratch(nx, ny, R):
    profile = CR.distinct_profile(R)
    for name, cells, threshold in RR.layers(nx, ny):
        cost_old = CR.cost_separable(cells, threshold, R, profile, FREE)
        for k, (dx, dy) in enumerate(RR.shifts(nx, ny)):
            for source in ("strips", "fill"):
                if source == "strips":
                    strips = RR.strips_of(window(nx, ny, k), dx, dy)
                    new = RR.roll_layer(cells, dx, dy, strips=strips)
                else:   # (fill: occupied under every threshold of the list)
                    new = RR.roll_layer(cells, dx, dy, fill=255 if k % 2 else 0)
                got = RR.roll_cost(cost_old, new, dx, dy, threshold, R, profile, FREE)
                assert same(got, CR.cost_separable(new, threshold, R, profile, FREE)), (name, dx, dy, source)


def test_roll_layer_is_the_spec_cell_by_cell():
    nx, ny = 7, 5
    cells = np.arange(nx * ny, dtype=np.uint8).reshape(ny, nx) + 1
    win = np.arange(nx * ny, dtype=np.uint8).reshape(ny, nx) + 101
    for dx, dy in RR.shifts(nx, ny):
        got = RR.roll_layer(cells, dx, dy, strips=RR.strips_of(win, dx, dy))
        filled = RR.roll_layer(cells, dx, dy, fill=9)
        for iy in range(ny):
            for ix in range(nx):
                inside = 0 <= ix + dx < nx and 0 <= iy + dy < ny
                assert got[iy, ix] == (cells[iy + dy, ix + dx] if inside else win[iy, ix])
                assert filled[iy, ix] == (cells[iy + dy, ix + dx] if inside else 9)
                assert RR.exposed_mask(nx, ny, dx, dy)[iy, ix] == (not inside)
    assert same(RR.roll_layer(cells, 0, 0), cells)


def test_the_strip_layout_of_the_worked_example():
    """the header's 5 x 4 map rolled by (2, -1): row 0, then the columns 3 and 4 of the rows 1, 2, 3"""
    nx, ny = 5, 4
    win = (10 * np.arange(ny)[:, None] + np.arange(nx)[None, :]).astype(np.uint8)   # cell (ix, iy) holds 10 * iy + ix
    buf = RR.pack_strips([RR.strips_of(win, 2, -1)])
    assert buf.tolist() == [0, 1, 2, 3, 4, 13, 14, 23, 24, 33, 34]
    assert RR.pack_strips([RR.strips_of(win, -2, 1)]).tolist() == [30, 31, 32, 33, 34, 0, 1, 10, 11, 20, 21]
    sizes, moves = [(5, 4), (3, 3), (5, 4)], [(2, -1), (0, 0), (-9, 1)]
    wins = [win, win[:3, :3], win]
    entries = [RR.strips_of(w, dx, dy) for w, (dx, dy) in zip(wins, moves)]
    back = RR.unpack_strips(RR.pack_strips(entries), sizes, moves)
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(entries, back))
    assert back[1][0].size == back[1][1].size == 0 and back[2][0].shape == (1, 5) and back[2][1].shape == (3, 5)


def test_ten_rolls_in_a_row_and_the_origin_is_not_a_running_sum():
    nx, ny, R, res = 67, 45, 3, 0.05
    profile = CR.distinct_profile(R)
    rng = np.random.default_rng(11)
    cells = np.where(rng.random((ny, nx)) < 0.05, 200, 50).astype(np.uint8)
    cost = CR.cost_separable(cells, 128, R, profile, FREE)
    origin0, c, running = (-1.7, 0.3), [0, 0], [-1.7, 0.3]
    drifted = False
    for k in range(10):
        dx, dy = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
        new = RR.roll_layer(cells, dx, dy, strips=RR.strips_of(window(nx, ny, 100 + k), dx, dy))
        cost = RR.roll_cost(cost, new, dx, dy, 128, R, profile, FREE)
        cells = new
        c = [c[0] + dx, c[1] + dy]
        running = [running[0] + dx * res, running[1] + dy * res]
        assert same(cost, CR.cost_separable(cells, 128, R, profile, FREE)), k
        assert RR.rolled_origin(origin0, c, res) == (origin0[0] + c[0] * res, origin0[1] + c[1] * res)
        drifted |= tuple(running) != RR.rolled_origin(origin0, c, res)
    # the running sum is another number: one cell at a time from 0.0 at a resolution of 0.05
    ox = 0.0
    for k in range(1, 101):
        ox += res
        drifted |= ox != RR.rolled_origin((0.0, 0.0), (k, 0), res)[0]
    assert drifted


# ---- wrong versions ---------------------------------------------------------------------------------------------------------------
def corner_case(R):
    """occupied cells that a roll by (3, 2) pushes just out of the map, one in x alone (to new ix = -1: its ring reached ix = R - 1)
    and one in y alone, one that stays, and two that enter opposite"""
    nx, ny = 67, 45
    cells = np.zeros((ny, nx), dtype=np.uint8)
    cells[20, 2] = cells[1, 30] = cells[ny - 5, nx - 10] = 1
    win = np.zeros((ny, nx), dtype=np.uint8)
    win[ny - 1, nx - 2] = win[ny // 3, nx - 1] = 1
    profile = CR.distinct_profile(R)
    dx, dy = 3, 2
    new = RR.roll_layer(cells, dx, dy, strips=RR.strips_of(win, dx, dy))
    return cells, win, new, CR.cost_separable(cells, 1, R, profile, FREE), CR.cost_separable(new, 1, R, profile, FREE), profile, dx, dy


@pytest.mark.parametrize("R", (3, 17))
def test_narrower_bands_differ(R):
    cells, win, new, cost_old, want, profile, dx, dy = corner_case(R)
    assert same(RR.roll_cost(cost_old, new, dx, dy, 1, R, profile, FREE), want)
    for margins in (dict(trail=0), dict(trail=R - 1), dict(lead=0)):
        assert not same(RR.roll_cost(cost_old, new, dx, dy, 1, R, profile, FREE, **margins), want), margins
    # (and one cell more than needed changes nothing)
    assert same(RR.roll_cost(cost_old, new, dx, dy, 1, R, profile, FREE, lead=R + 1, trail=R + 1), want)


def test_a_flipped_shift_differs():
    cells, win, new, *_ , dx, dy = corner_case(3)
    assert not same(RR.roll_layer(cells, -dx, -dy, strips=RR.strips_of(win, -dx, -dy)), new)


def test_exposed_cells_left_at_their_old_content_differ():
    cells, win, new, *_, dx, dy = corner_case(3)
    stale = np.where(RR.exposed_mask(67, 45, dx, dy), cells, new)
    assert not same(stale, new)


def test_wrong_strip_layouts_differ():
    nx, ny, dx, dy = 5, 4, 2, -1
    win = (10 * np.arange(ny)[:, None] + np.arange(nx)[None, :]).astype(np.uint8)
    rows, cols = RR.strips_of(win, dx, dy)
    good = RR.pack_strips([(rows, cols)])
    swapped = np.concatenate([cols.reshape(-1), rows.reshape(-1)])
    every_row = np.concatenate([rows.reshape(-1), win[:, RR.strip_cols(nx, dx)].reshape(-1)])   # the column strip over all rows
    assert len(swapped) == len(good) and not np.array_equal(swapped, good)
    assert len(every_row) != len(good)
    old = np.zeros((ny, nx), dtype=np.uint8)
    want = RR.roll_layer(old, dx, dy, strips=(rows, cols))
    got = RR.roll_layer(old, dx, dy, strips=RR.unpack_strips(swapped, [(nx, ny)], [(dx, dy)])[0])
    assert not same(got, want)
    got = RR.roll_layer(old, dx, dy, strips=RR.unpack_strips(every_row[:len(good)], [(nx, ny)], [(dx, dy)])[0])
    assert not same(got, want)


def test_wrong_origins_differ():
    res, origin0 = 0.05, (1.25, -0.4)
    good = RR.rolled_origin(origin0, (3, -2), res)
    assert good == (1.25 + 3.0 * 0.05, -0.4 + -2.0 * 0.05)
    assert RR.rolled_origin(origin0, (-3, 2), res) != good                       # the opposite sign
    # repeated addition drifts at a resolution like 0.05: within 1000 single-cell rolls it has left the exact form
    ox, left = origin0[0], None
    for k in range(1, 1001):
        ox += res
        if left is None and ox != RR.rolled_origin(origin0, (k, 0), res)[0]:
            left = k
    assert left is not None and left <= 1000

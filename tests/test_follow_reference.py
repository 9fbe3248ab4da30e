"""CPU tests of the follow decision (tests/follow_reference.py): the statement at its edges, the origin
formula against exact rational arithmetic, every listed mutation caught by a listed case, numpy's batch.follow_shift equal to the
statement, and what the device decides with -- follow_decide (csrc/mppi_costmap_follow_decide.h) and roll_bands
(csrc/mppi_costmap_rects.h), compiled into a stand-alone host program (tools/costmap_follow_check.cpp) -- equal to it too.  The
limit of 2^30 accumulated cells is held here only: reaching it on the device takes about 10^5 calls.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import follow_reference as FR
from ccv_mppi_path_tracker_amd import batch, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.25
GEO = ((-3.0, 1.5), RES, 9, 6)      # nx odd, ny even: centre cells 4 and 3
F0 = (0, 0, -3.0, 1.5)


def at(cell, frac=(0.5, 0.5), frame=F0, geo=GEO):
    return FR.pose_for(frame, geo, cell, frac)


# (name, frame, pose, geometry, margin, max_step, expected (status, dx, dy))
CASES = [
    ("centre", F0, at((4, 3)), GEO, 0, 5, (FR.HELD, 0, 0)),
    ("e_equals_margin", F0, at((6, 3)), GEO, 2, 5, (FR.HELD, 0, 0)),
    ("e_is_margin_plus_one", F0, at((7, 3)), GEO, 2, 5, (FR.MOVED, 3, 0)),
    ("minus_margin_and_minus_margin_minus_one", F0, at((2, 0)), GEO, 2, 5, (FR.MOVED, 0, -3)),
    ("clamped_at_max_step", F0, at((40, 3)), GEO, 2, 5, (FR.MOVED, 5, 0)),
    ("clamped_below", F0, at((4, -40)), GEO, 0, 7, (FR.MOVED, 0, -7)),
    ("max_step_exactly", F0, at((9, 3)), GEO, 1, 5, (FR.MOVED, 5, 0)),
    ("on_a_cell_edge", F0, at((7, 3), (0.0, 0.0)), GEO, 2, 5, (FR.MOVED, 3, 0)),
    ("just_below_the_edge", F0, (np.nextafter(at((7, 3), (0.0, 0.0))[0], -np.inf), at((7, 3))[1]), GEO, 2, 5, (FR.HELD, 0, 0)),
    ("left_of_the_map_floor", F0, at((-1, 3), (0.5, 0.5)), GEO, 4, 9, (FR.MOVED, -5, 0)),     # floor(-0.5) = -1: e = -5; trunc: e = -4
    ("below_the_map_floor", F0, at((4, -1), (0.5, 0.25)), GEO, 3, 9, (FR.MOVED, 0, -4)),
    ("both_axes_opposite_signs", F0, at((8, 0)), GEO, 1, 9, (FR.MOVED, 4, -3)),
    ("one_axis_moves_the_other_is_inside", F0, at((8, 4)), GEO, 1, 9, (FR.MOVED, 4, 0)),
    ("nan_x", F0, (np.nan, 2.0), GEO, 1, 9, (FR.NO_POSE, 0, 0)),
    ("nan_y", F0, (0.0, np.nan), GEO, 1, 9, (FR.NO_POSE, 0, 0)),
    ("plus_inf", F0, (np.inf, 2.0), GEO, 1, 9, (FR.NO_POSE, 0, 0)),
    ("minus_inf", F0, (0.0, -np.inf), GEO, 1, 9, (FR.NO_POSE, 0, 0)),
    ("fx_is_2_to_30", (0, 0, 0.0, 0.0), (2.0 ** 30 * RES, 0.0), ((0.0, 0.0), RES, 9, 6), 1, 9, (FR.NO_POSE, 0, 0)),
    ("fx_just_below_2_to_30", (0, 0, 0.0, 0.0), (np.nextafter(2.0 ** 30 * RES, 0.0), 0.0), ((0.0, 0.0), RES, 9, 6), 1, 9, (FR.MOVED, 9, -3)),
    ("fx_is_minus_2_to_30", (0, 0, 0.0, 0.0), (0.0, -(2.0 ** 30) * RES), ((0.0, 0.0), RES, 9, 6), 1, 9, (FR.NO_POSE, 0, 0)),
    ("offset_at_the_limit_moves", (2 ** 30 - 3, 0, -3.0 + (2 ** 30 - 3) * RES, 1.5), None, GEO, 2, 5, (FR.MOVED, 3, 0)),
    ("offset_beyond_the_limit", (2 ** 30 - 2, 0, -3.0 + (2 ** 30 - 2) * RES, 1.5), None, GEO, 2, 5, (FR.LIMIT, 0, 0)),
    ("offset_beyond_the_limit_below", (0, -(2 ** 30), -3.0, 1.5 - 2 ** 30 * RES), "down", GEO, 2, 5, (FR.LIMIT, 0, 0)),
    ("one_by_one_held", (0, 0, 0.0, 0.0), (0.125, 0.125), ((0.0, 0.0), RES, 1, 1), 0, 3, (FR.HELD, 0, 0)),
    ("one_by_one_moves", (0, 0, 0.0, 0.0), (0.3, -0.01), ((0.0, 0.0), RES, 1, 1), 0, 3, (FR.MOVED, 1, -1)),
    ("even_by_odd", (0, 0, 0.0, 0.0), (RES * 3.5, RES * 3.5), ((0.0, 0.0), RES, 4, 5), 0, 9, (FR.MOVED, 1, 1)),   # centres 2, 2
    ("a_rolled_frame", (7, -2, -3.0 + 7 * RES, 1.5 - 2 * RES), None, GEO, 1, 2, (FR.MOVED, 2, 0)),
]


def resolve(case):
    name, frame, pose, geo, margin, max_step, want = case
    if pose is None:   # three cells right of the centre of the frame as it is
        pose = FR.pose_for(frame, geo, (7, 3))
    elif isinstance(pose, str):   # three cells below it
        pose = FR.pose_for(frame, geo, (4, 0))
    return name, frame, pose, geo, margin, max_step, want


RESOLVED = [resolve(c) for c in CASES]


@pytest.mark.parametrize("case", RESOLVED, ids=[c[0] for c in RESOLVED])
def test_the_decision_at_its_edges(case):
    name, frame, pose, geo, margin, max_step, want = case
    status, dx, dy, new = FR.decide(frame, pose, geo, margin, max_step)
    assert (status, dx, dy) == want
    if status == FR.MOVED:
        (ox0, oy0), res, _, _ = geo
        assert new[:2] == (frame[0] + dx, frame[1] + dy)
        assert new[2] == FR.rolled_origin_exact(ox0, new[0], res) and new[3] == FR.rolled_origin_exact(oy0, new[1], res)
    else:
        assert new == frame


def test_the_origin_formula_against_exact_rational_arithmetic():
    rng = np.random.default_rng(5)
    for res in (0.05, 0.1, 0.25, 1.0 / 3.0, 0.3):
        for origin0 in (0.0, -3.0, 1.0e6 / 3.0, -12.345678901234567):
            for c in [0, 1, -1, 2 ** 30, -(2 ** 30)] + [int(v) for v in rng.integers(-2 ** 30, 2 ** 30, 40)]:
                assert origin0 + float(c) * res == FR.rolled_origin_exact(origin0, c, res), (res, origin0, c)
    # the statement never drifts: 1000 moves of one cell land on the same bits as one look at the count; a running sum does not
    geo, frame, drift = ((0.1, -0.7), 0.1, 9, 6), (0, 0, 0.1, -0.7), (0, 0, 0.1, -0.7)
    for _ in range(1000):
        frame = FR.decide(frame, FR.pose_for(frame, geo, (5, 3)), geo, 0, 1)[3]
        drift = FR.decide(drift, FR.pose_for(drift, geo, (5, 3)), geo, 0, 1, wrong="origin_sum")[3]
    assert frame == (1000, 0, 0.1 + 1000.0 * 0.1, -0.7) and drift[0] == 1000 and drift[2] != frame[2]


@pytest.mark.parametrize("wrong", FR.MUTATIONS)
def test_every_mutation_differs_on_a_listed_case(wrong):
    assert len(FR.MUTATIONS) >= 6
    caught = []
    for name, frame, pose, geo, margin, max_step, want in RESOLVED:
        spec = FR.decide(frame, pose, geo, margin, max_step)
        if FR.decide(frame, pose, geo, margin, max_step, wrong=wrong) != spec:
            caught.append(name)
    if wrong == "origin_sum":   # (one move from an exact frame gives the same bits: the drift test above is its listed case)
        geo, a, b = ((0.1, -0.7), 0.1, 9, 6), (0, 0, 0.1, -0.7), (0, 0, 0.1, -0.7)
        for _ in range(1000):
            a = FR.decide(a, FR.pose_for(a, geo, (5, 3)), geo, 0, 1)[3]
            b = FR.decide(b, FR.pose_for(b, geo, (5, 3)), geo, 0, 1, wrong=wrong)[3]
        caught += ["drift"] * (a != b)
    assert caught, wrong


def test_numpys_follow_shift_is_the_statement():
    for name, frame, pose, geo, margin, max_step, want in RESOLVED:
        (ox0, oy0), res, nx, ny = geo
        got = batch.follow_shift(((frame[2], frame[3]), res, nx, ny), [pose], margin, max_step)
        status, dx, dy, _ = FR.decide(frame, pose, geo, margin, max_step)
        if status == FR.LIMIT:   # (the accumulated limit is the roll's own check, not the shift's)
            continue
        assert got.dtype == np.int32 and got.tolist() == [[dx, dy]], name


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("follow") / "costmap_follow_check")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", build.CSRC, os.path.join(ROOT, "tools", "costmap_follow_check.cpp"), "-o", out], check=True)
    return out


def test_the_devices_decision_is_the_statement(check_program):
    rng = np.random.default_rng(11)
    cases = [(frame, pose, geo, margin, max_step) for _, frame, pose, geo, margin, max_step, _ in RESOLVED]
    for _ in range(400):   # poses round a small map, resolutions that are no powers of two
        res = float(rng.choice([0.05, 0.1, 0.3, 0.25]))
        nx, ny = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        o0 = (float(rng.normal()), float(rng.normal()))
        cx, cy = int(rng.integers(-50, 50)), int(rng.integers(-50, 50))
        frame = (cx, cy, o0[0] + float(cx) * res, o0[1] + float(cy) * res)
        pose = (frame[2] + float(rng.uniform(-3, nx + 3)) * res, frame[3] + float(rng.uniform(-3, ny + 3)) * res)
        cases.append((frame, pose, (o0, res, nx, ny), int(rng.integers(0, 4)), int(rng.integers(1, 6))))
    lines = ["%d %d %s %s %s %s %s %s %s %d %d %d %d" % (f[0], f[1], float(f[2]).hex(), float(f[3]).hex(), float(p[0]).hex(), float(p[1]).hex(),
                                                         float(g[0][0]).hex(), float(g[0][1]).hex(), float(g[1]).hex(), g[2], g[3], m, s)
             for f, p, g, m, s in cases]
    out = subprocess.run([check_program, "decide"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(cases) + 1
    for (f, p, g, m, s), line in zip(cases, out):
        status, dx, dy, new = FR.decide(f, p, g, m, s)
        w = line.split()
        got = (int(w[0]), int(w[1]), int(w[2]), (int(w[3]), int(w[4]), float.fromhex(w[5]), float.fromhex(w[6])))
        assert got == (status, dx, dy, tuple(new)), (f, p, g, m, s)


def test_the_band_arithmetic_of_device_and_host_is_one_statement_and_equals_the_restatement(check_program):
    out = subprocess.run([check_program, "bands", "9", "10", "3"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 9 * 9 * 21 * 21 * 4
    for line in out:
        v = [int(t) for t in line.split()]
        nx, ny, ex, ey, R, n = v[:6]
        want = FR.bands(nx, ny, ex, ey, R)
        assert n == len(want) and [tuple(v[6 + 4 * k:10 + 4 * k]) for k in range(n)] == want, line
    # one statement: the kernel unit and the host unit include the same header, and nothing else defines the bands
    holders = [f for f in sorted(os.listdir(build.CSRC)) if f.endswith((".h", ".hip")) and "int roll_bands(" in open(os.path.join(build.CSRC, f)).read()]
    assert holders == ["mppi_costmap_rects.h"]
    for unit in ("k_costmap_follow.hip", "capi_batch_maps.hip"):
        text = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "mppi_costmap_rects.h"' in text and "roll_bands(" in text, unit

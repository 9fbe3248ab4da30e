"""CPU pins of the fleet term's checker (tests/fleet_reference.py): the numpy float64 selection against
the exact-rational one over the edge shapes, six wrong versions that must each differ on at least one of those cases, and the
three entry points in the library.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import fleet_reference as FR
from ccv_mppi_path_tracker_amd import capi

MAXN = FR.MAX_OBSTACLES
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _case(name, q, radius, n_static, max_neighbours, rng, q_post=None):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
    B = len(q)
    q_post = q + np.array([0.013, -0.007]) * (1 + np.arange(B))[:, None] if q_post is None else np.asarray(q_post, dtype=np.float64)
    return dict(name=name, q=q, q_post=q_post, radius=np.broadcast_to(np.asarray(radius, dtype=np.float64), (B,)).copy(),
                n_static=np.broadcast_to(np.asarray(n_static, dtype=np.int32), (B,)).copy(), maxn=int(max_neighbours), rng=float(rng))


def cases():
    out = []
    g = np.random.default_rng(20260)
    for i, (B, maxn) in enumerate(((12, 2), (40, 32), (7, 1), (33, 4))):   # random fleets; n_static dealt from {0, 30, 32}
        out.append(_case("random%d" % i, g.uniform(0.0, 5.0, (B, 2)), g.uniform(0.1, 0.6, B), g.choice([0, 30, 32], B), maxn,
                         (1.7, 9.0, 2.5, 1.2)[i]))
    # exact ties: robots 1 and 2 symmetric about robot 0, robot 3 at the same distance on the other axis
    tie = [[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.25, 0.25]]
    for maxn in (1, 2, 32):
        out.append(_case("ties_m%d" % maxn, tie, [0.3, 0.2, 0.25, 0.35, 0.15], 0, maxn, 2.0))
    out.append(_case("ties_room1", tie, 0.3, [31, 0, 30, 32, 0], 3, 2.0))
    # a robot exactly on the range: d2 = 25 = range2; the other one a last place beyond
    out.append(_case("on_range", [[0.0, 0.0], [3.0, 4.0], [0.0, -np.nextafter(5.0, 6.0)]], [0.4, 0.1, 0.2], 0, 2, 5.0))
    # M_y = 0 (a full static list), 1, 2 and 32 (the cap of 32 below the 39 robots in range)
    grid = np.stack(np.meshgrid(np.arange(8) * 0.5, np.arange(5) * 0.5), axis=-1).reshape(-1, 2)
    out.append(_case("grid_m32", grid, np.linspace(0.1, 0.5, len(grid)), 0, 32, 100.0))
    out.append(_case("grid_m0_1_2", grid, 0.2, np.array([32, 31, 30, 0] * 10), 2, 1.0))
    out.append(_case("nobody_in_range", [[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]], 0.3, [0, 30, 32], 2, 0.0))
    out.append(_case("single", [[1.5, -2.0]], 0.3, 0, 4, 10.0))
    return out


CASES = cases()


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_float64_and_exact_rational_selection_agree(c):
    a = FR.lists(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"])
    b = FR.lists_exact(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"])
    assert same(a, b), c["name"]
    M = FR.room(c["n_static"], c["maxn"])
    for y, r in enumerate(a[1]):
        assert len(r) <= M[y] and a[0][y] == c["n_static"][y] + len(r) <= MAXN


def test_the_edge_shapes_are_what_they_claim():
    by = {c["name"]: c for c in CASES}
    n, rows = FR.lists(*[by["ties_m1"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert rows[0].tolist() == [[0.25, 0.25, 0.3 + 0.15]]          # the nearest
    n, rows = FR.lists(*[by["ties_m32"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert [tuple(r[:2]) for r in rows[0]] == [(0.25, 0.25), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0)]   # equal d2: the lower index first
    assert rows[0][1, 2] == 0.3 + 0.2
    n, rows = FR.lists(*[by["on_range"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert n.tolist() == [1, 1, 0] and rows[0][0, :2].tolist() == [3.0, 4.0]      # on the range: in; a last place beyond: out
    n, rows = FR.lists(*[by["grid_m32"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert n.tolist() == [32] * 40
    c = by["grid_m0_1_2"]
    n, rows = FR.lists(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"])
    assert sorted(set((n - c["n_static"]).tolist())) == [0, 1, 2] and n.max() == 32
    n, rows = FR.lists(*[by["nobody_in_range"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert n.tolist() == [0, 30, 32] and all(len(r) == 0 for r in rows)
    n, rows = FR.lists(*[by["single"][k] for k in ("q", "radius", "n_static", "maxn", "rng")])
    assert n.tolist() == [0] and rows[0].shape == (0, 3)
    # a NaN position is nobody's candidate and has none (float64 backend only: a NaN is no rational)
    q = np.array([[0.0, 0.0], [np.nan, 0.0], [1.0, 0.0]])
    n, rows = FR.lists(q, [0.1, 0.1, 0.1], [0, 0, 0], 2, 5.0)
    assert n.tolist() == [1, 0, 1] and rows[0][0, 0] == 1.0 and rows[2][0, 0] == 0.0


def wrong(kind, c):
    """the selection with one mistake"""
    q, qp, radius, ns, rng = c["q"], c["q_post"], c["radius"], c["n_static"], c["rng"]
    B = len(q)
    M = FR.room(ns, c["maxn"])
    range2 = np.float64(rng) * np.float64(rng)
    n_total, rows = np.zeros(B, dtype=np.int32), []
    for y in range(B):
        centre = qp[y] if kind == "own_post_advance_position" else q[y]
        pool = [j for j in range(B) if j != y or kind == "self_not_excluded"]
        if kind == "cap_before_range":   # only the first M_y robots (by index) are looked at
            pool = pool[:M[y]]
        cands = []
        for j in pool:
            dx, dy = q[j, 0] - centre[0], q[j, 1] - centre[1]
            d2 = dx * dx + dy * dy
            if (d2 < range2) if kind == "strict_range" else (d2 <= range2):
                cands.append((d2, -j if kind == "ties_to_higher_index" else j, j))
        take = [j for _, _, j in sorted(cands)[:M[y]]]
        rows.append(np.array([[q[j, 0], q[j, 1], radius[j] if kind == "radius_of_j_alone" else radius[y] + radius[j]]
                              for j in take]).reshape(-1, 3))
        n_total[y] = int(ns[y]) + len(take)
    return n_total, rows


WRONG = ("self_not_excluded", "strict_range", "ties_to_higher_index", "cap_before_range", "radius_of_j_alone",
         "own_post_advance_position")


def test_the_restatement_without_a_mistake_is_the_reference():
    for c in CASES:
        assert same(wrong(None, c), FR.lists(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"])), c["name"]


@pytest.mark.parametrize("kind", WRONG)
def test_a_wrong_version_differs_on_some_case(kind):
    differs = [c["name"] for c in CASES if not same(wrong(kind, c), FR.lists(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"]))]
    print(kind, "differs on", differs)
    assert differs


FLEET = ("ccv_mppi_batch_resident_set_fleet", "ccv_mppi_batch_resident_get_fleet", "ccv_mppi_batch_resident_read_fleet")


def test_the_library_exports_the_fleet_entry_points_and_refuses_a_null_handle():
    lib = capi.load()
    for name in FLEET:
        assert name in capi.FLEET_SIGNATURES and hasattr(lib, name), name
    r = np.ones(2)
    assert lib.ccv_mppi_batch_resident_set_fleet(None, capi.dptr(r), 1.0, 2, capi.dptr(r)) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_get_fleet(None, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_resident_read_fleet(None, None, None, None) == capi.ERR_INVALID_ARG


def test_the_fleet_header_declares_exactly_the_ctypes_table_and_compiles_as_c99_from_either_include(tmp_path):
    """The three calls live in include/ccv_mppi_fleet.h, which ccv_mppi.h includes: the header's names are the ctypes table's,
    no table holds a name twice, and a C99 caller gets the prototypes from either header."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "ccv_mppi_fleet.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(ccv_mppi_[a-z_0-9]+)\s*\(", src)) == set(FLEET) == set(capi.FLEET_SIGNATURES)
    assert not set(capi.FLEET_SIGNATURES) & set(capi.SIGNATURES)
    for header in ("ccv_mppi.h", "ccv_mppi_fleet.h"):
        c = tmp_path / ("fleet_%s.c" % header[:-2])
        c.write_text('#include <stddef.h>\n#include "%s"\n' % header +
                     'typedef int (*set_fn)(ccv_mppi_batch*, const double*, double, int32_t, const double*);\n'
                     'typedef int (*get_fn)(ccv_mppi_batch*, double*, double*, int32_t*);\n'
                     'typedef int (*read_fn)(ccv_mppi_batch*, int32_t*, int32_t*, double*);\n'
                     'int main(void){set_fn a = ccv_mppi_batch_resident_set_fleet; get_fn b = ccv_mppi_batch_resident_get_fleet;\n'
                     'read_fn c = ccv_mppi_batch_resident_read_fleet; return (a && b && c && CCV_MPPI_MAX_OBSTACLES >= 1) ? 0 : 1;}\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", INCLUDE, str(c), "-o", str(c) + ".o"],
                       check=True)

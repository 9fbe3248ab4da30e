"""CPU pins of the fleet term's checker (tests/fleet_reference.py): the numpy float64 selection against
the exact-rational one over the edge shapes, six wrong versions that must each differ on at least one of those cases, and the
three entry points in the library.  No GPU."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fleet_cases as FC
import fleet_reference as FR
from ccv_mppi_path_tracker_amd import capi
from fleet_cases import CASES, NEW, WRONG, same, wrong

MAXN = FR.MAX_OBSTACLES
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


FINITE = [c for c in CASES if c["finite"]]   # (a NaN or an infinity is no rational: those cases have the float64 backend only)


@pytest.mark.parametrize("c", FINITE, ids=[c["name"] for c in FINITE])
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


_REF = {}


def ref(c, step=0):
    """fleet_reference.lists of a case's position set, computed once"""
    if (c["name"], step) not in _REF:
        _REF[(c["name"], step)] = FR.lists(*FC.args(c, FC.positions(c)[step]))
    return _REF[(c["name"], step)]


def test_the_restatement_without_a_mistake_is_the_reference():
    for c in CASES:
        assert same(wrong(None, c), FR.lists(c["q"], c["radius"], c["n_static"], c["maxn"], c["rng"])), c["name"]


# the new wrong versions, and the new case that has to catch each (DESIGN.md section 10f holds the same table)
CAUGHT_BY = {"d2_fma_x": ("sym_pairs", "on_range_rounded"), "d2_fma_y": ("sym_pairs", "on_range_rounded"),
             "ties_by_thread_order": ("cross_stride_ties",), "count_of_one_wave": ("counts_across_waves_cap",),
             "first_block_only": ("cross_stride_ties", "block_sizes_B513", "block_sizes_B1024"),
             "nan_key_is_zero": ("not_finite_ordinary", "not_finite_huge")}


@pytest.mark.parametrize("kind", WRONG)
def test_a_wrong_version_differs_on_some_case(kind):
    differs = [c["name"] for c in CASES if not same(wrong(kind, c), ref(c))]
    print(kind, "differs on", differs)
    assert differs
    assert set(CAUGHT_BY.get(kind, ())) <= set(differs), kind
    if kind in CAUGHT_BY:   # (no case of the first change catches a new wrong version: the new cases are what holds them)
        assert not set(differs) - {c["name"] for c in NEW}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def test_the_second_position_set_agrees_between_the_backends_and_with_the_restatement():
    c = by_name("shrinking")
    a = ref(c, 1)
    assert same(a, FR.lists_exact(*FC.args(c, c["q_next"]))) and same(a, wrong(None, c, c["q_next"]))
    taken = [(ref(c, s)[0] - c["n_static"]).tolist() for s in (0, 1)]
    assert taken == [[4] * 10, [1] * 10]                  # every robot: four neighbours, then one
    assert [c["name"] for c in CASES if c["q_next"] is not None] == ["shrinking"]


def test_sym_pairs_flip_under_either_contraction_and_tie_without():
    c = by_name("sym_pairs")
    pairs = c["info"]["pairs"]
    n, rows = ref(c)
    flips = {"x": 0, "y": 0}
    assert len(pairs) == 8 and sorted(p["a_low"] for p in pairs) == [False] * 4 + [True] * 4 and c["maxn"] == 1
    for p in pairs:
        o, lo, hi = p["observer"], p["low"], p["high"]
        assert float(c["q"][o, 0]).hex().rstrip("0").count("") > 10    # (the observer's coordinate is not dyadic: a long mantissa)
        d_lo, x_lo, y_lo = FC.d2_forms(c["q"][lo], c["q"][o])
        d_hi, x_hi, y_hi = FC.d2_forms(c["q"][hi], c["q"][o])
        assert d_lo == d_hi and (x_lo, y_lo) == (y_hi, x_hi)           # the spec's keys tie to the bit: the lower index wins
        assert n[o] == 1 and rows[o][0, :2].tolist() == c["q"][lo].tolist()
        assert (x_hi < x_lo) != (y_hi < y_lo)                          # contracted, the higher index wins in exactly one form
        flips["x" if x_hi < x_lo else "y"] += 1
        assert p["flips"] == ("x" if x_hi < x_lo else "y")
    print("sym_pairs: pairs whose winner flips under fma(dx,dx,dy*dy) / fma(dy,dy,dx*dx): %d / %d; %d of %d random pairs had "
          "different contracted keys" % (flips["x"], flips["y"], c["info"]["sensitive"], c["info"]["tried"]))
    assert flips["x"] >= 1 and flips["y"] >= 1
    for kind, form in (("d2_fma_x", "x"), ("d2_fma_y", "y")):          # ... and the wrong version's row is the other robot
        _, wrows = wrong(kind, c)
        for p in pairs:
            assert wrows[p["observer"]][0, :2].tolist() == c["q"][p["high"] if p["flips"] == form else p["low"]].tolist()


def test_on_range_rounded_sits_on_the_rounded_range():
    c = by_name("on_range_rounded")
    kinds, range2 = c["info"]["kinds"], c["info"]["range2"]
    assert c["rng"] == 0.7 and range2 == 0.7 * 0.7 and Fraction(range2) != Fraction(0.7) ** 2    # (range2 is a rounded product)
    assert kinds.count("x") >= 1 and kinds.count("y") >= 1 and kinds.count("out") == 1 and kinds.count("plain") >= 1
    n, rows = ref(c)
    for j, kind in enumerate(kinds, start=1):
        d, fx, fy = FC.d2_forms(c["q"][j], c["q"][0])
        if kind == "out":
            assert d == np.nextafter(range2, np.inf)
        else:
            assert d == range2
            assert (fx > range2) == (kind == "x") and (kind != "y" or fy > range2)
    ins = [j for j, kind in enumerate(kinds, start=1) if kind != "out"]
    assert n[0] == len(ins) and rows[0][:, :2].tolist() == c["q"][ins].tolist()    # (equal keys: index order)
    for kind, form in (("d2_fma_x", "x"), ("d2_fma_y", "y")):
        assert wrong(kind, c)[0][0] < n[0]
    print("on_range_rounded: %d angles tried, exact hits %s" % (c["info"]["tried"], c["info"]["hits"]))


def test_cross_stride_ties_separate_thread_order_from_index_order():
    c = by_name("cross_stride_ties")
    differ = c["info"]["differ"]
    print("cross_stride_ties: %d robots whose two orders take different rows" % len(differ))
    assert len(c["q"]) == 600 and c["maxn"] == 2 and len(differ) >= 50
    n, rows = ref(c)
    _, wrows = wrong("ties_by_thread_order", c)
    K = FC.KBLOCK
    for y in differ:
        d2 = np.sum((c["q"] - c["q"][y]) ** 2, axis=1)
        tied = [j for j in np.flatnonzero(d2 == 0.0625)]
        assert len(tied) >= 3 and np.sum(d2 <= 0.09) == len(tied) + 1             # an exact tie at the cap of 2
        assert any(a % K < b % K and a > b for a in tied for b in tied)              # the smaller j % 256 with the larger j
        assert rows[y].tobytes() != wrows[y].tobytes()
    assert (n == c["n_static"] + np.minimum(2, [np.sum(np.sum((c["q"] - p) ** 2, axis=1) <= 0.09) - 1 for p in c["q"]])).all()


def test_counts_across_waves_name_robots_below_at_and_above_the_cap():
    a, c = by_name("counts_across_waves_all"), by_name("counts_across_waves_cap")
    assert len(a["q"]) == len(c["q"]) == 1024 and sorted(set(a["n_static"].tolist())) == [0, 30, 31, 32]
    n, rows = ref(a)
    assert (n == 32).all() and sorted({len(r) for r in rows}) == [0, 1, 2, 32]       # 1023 candidates each: M_y rows
    n, rows = ref(c)
    named = c["info"]["named"]
    assert sorted(named) == ["above", "at", "below"]
    for key, count in (("below", 2), ("at", 3), ("above", 4)):
        y, cand = named[key]["robot"], np.array(named[key]["candidates"])
        d2 = np.sum((c["q"] - c["q"][y]) ** 2, axis=1)
        assert sorted(np.flatnonzero((d2 <= 0.3 * 0.3) & (np.arange(1024) != y)).tolist()) == sorted(cand.tolist())
        assert len(cand) == count == c["maxn"] + {"below": -1, "at": 0, "above": 1}[key] and n[y] == min(count, 3)
        assert len(set(cand // 64)) == count == len(set((cand % FC.KBLOCK) // 64)) and (cand // 64).min() > 0
        assert wrong("count_of_one_wave", c)[0][y] == 0


def test_block_sizes_surround_every_multiple_of_the_wave_and_the_workgroup():
    names = [c["name"] for c in CASES if c["name"].startswith("block_sizes_")]
    assert names == ["block_sizes_B%d" % B for B in (2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)]
    for name in names:
        c = by_name(name)
        n, rows = ref(c)
        assert len(c["q"]) == int(name.split("B")[-1])
        taken = n - c["n_static"]
        assert (taken == np.minimum(FR.room(c["n_static"], 4), taken)).all() and taken.max() == min(4, len(c["q"]) - 1)
    assert sum(len(c["q"]) == 1024 for c in CASES) == 3                                # (the largest batch: three cases in all)


def test_not_finite_positions_give_what_the_case_states():
    for name in ("not_finite_ordinary", "not_finite_huge"):
        c = by_name(name)
        assert not c["finite"] and np.isnan(c["q"]).sum() == 2 and np.isinf(c["q"]).sum() == 2 and np.nanmax(np.abs(c["q"])) == np.inf
        n, rows = ref(c)
        for y, want in c["info"]["expect"].items():
            got = [int(np.flatnonzero([r.tobytes() == p.tobytes() for p in c["q"]])[0]) for r in rows[y][:, :2]]
            assert sorted(got) == sorted(want) and n[y] == len(want), (name, y, got)
            assert got[len(got) - len([j for j in want if j >= 8]):] == [j for j in want if j >= 8]   # equal keys of +inf: index order
    huge = by_name("not_finite_huge")
    with np.errstate(over="ignore"):
        assert np.float64(huge["rng"]) * np.float64(huge["rng"]) == np.inf and np.isfinite(huge["rng"])


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

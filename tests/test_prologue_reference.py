"""CPU tests of tests/prologue_reference.py: the restatement of get_CurrentIndex() + calc_RefPath() equals the product's host
prologue (ccv_mppi_calc_ref_path) and the oracle's restatement of the reference bit for bit over the whole case list, every
case has the property it is named for, and every wrong version in MUTATIONS is told apart by at least one case."""
import math

import numpy as np
import pytest

import ccv_mppi_path_tracker_amd as amd
from oracle import oracle_lib as O
import prologue_reference as PR

CASES = PR.cases()
LAYOUT = PR.batch_layout()


def by_group(group):
    return [c for c in CASES if c["group"] == group]


def window(c, fn=PR.ref_window):
    return fn(c["px"], c["py"], c["x"], c["y"], c["v_ref"], c["dt"], c["resolution"], c["H"])


def layout_arrays():
    px = np.concatenate([p[0] for p in LAYOUT["paths"]])
    py = np.concatenate([p[1] for p in LAYOUT["paths"]])
    return px, py


def test_restatement_equals_host_prologue_and_oracle_on_every_case():
    cases = list(CASES)
    for b, (px, py) in enumerate(LAYOUT["paths"]):
        for H in (9, 30):
            cases.append(dict(name="layout%d" % b, px=px, py=py, x=LAYOUT["poses"][b][0], y=LAYOUT["poses"][b][1], H=H, expect=LAYOUT["expect"][b],
                              v_ref=LAYOUT["v_ref"][b], dt=LAYOUT["dt"], resolution=LAYOUT["resolution"][b]))
    for c in cases:
        idx, xr, yr, (s0, s1) = window(c)
        assert idx == c["expect"], c["name"]
        for lib in (amd, O):
            i2, xr2, yr2, yaw2 = lib.calc_ref_path(c["px"], c["py"], c["x"], c["y"], c["v_ref"], c["dt"], c["resolution"], c["H"])
            assert i2 == idx, (c["name"], lib.__name__)
            np.testing.assert_array_equal(xr2, xr, err_msg=c["name"])
            np.testing.assert_array_equal(yr2, yr, err_msg=c["name"])
            assert yaw2[0] == math.atan2(c["py"][s1] - c["py"][s0], c["px"][s1] - c["px"][s0]), c["name"]   # (libm, as both libraries)
            assert s0 != s1 or yaw2[0] == 0.0


def test_case_list_covers_what_the_issue_names():
    lens = {len(c["px"]) for c in by_group("length")}
    assert lens == set(PR.LENGTHS)
    for n in PR.LENGTHS:
        got = {c["expect"] for c in by_group("length") if len(c["px"]) == n}
        top = ((n - 1) // 256) * 256
        assert got == {j for j in (0, n - 1, top - 1, top, top + 1) if 0 <= j < n}
    assert max(len(c["px"]) for c in CASES) <= 3 * 4096
    assert {c["H"] for c in CASES} == {9, 30}
    assert {(c["v_ref"], c["dt"], c["resolution"]) for c in by_group("stride")} == set(PR.STRIDES)
    assert any(c["moving"] for c in by_group("tie")) and any(c["moving"] for c in by_group("end"))


def test_every_other_pose_is_strictly_farther():
    for c in CASES:
        d = PR.distances(c["px"], c["py"], c["x"], c["y"])
        if c["group"] == "gate":
            assert np.all(np.delete(d, 5) > 2 * PR.GATE), c["name"]
        elif c["group"] in ("same_sqrt", "one_ulp"):
            assert np.sum(d < PR.GATE) == 2, c["name"]
        else:
            near = d.min()
            assert near < 0.05 or len(d) == 1, c["name"]
            assert np.all(d[d != near] > near + 0.01), c["name"]
            assert d[c["expect"]] == near and not np.any(d[:c["expect"]] == near), c["name"]


def thread_of(i, nt):
    return i % nt, (i % nt) // 64, i % 64, i // (PR.K_LOADS * nt)      # thread, wave, lane, outer round


def test_tie_cases_are_exact_ties_in_every_thread_arrangement():
    seen = {nt: set() for nt in PR.NTS}
    for c in by_group("tie"):
        d = PR.distances(c["px"], c["py"], c["x"], c["y"])
        tied = np.flatnonzero(d == d.min())
        assert len(tied) >= 2 and tied[0] == c["expect"], c["name"]
        assert all(c["px"][i] == c["px"][tied[0]] and c["py"][i] == c["py"][tied[0]] for i in tied), c["name"]
        for nt in PR.NTS:
            t0, w0, l0, r0 = thread_of(tied[0], nt)
            for i in tied[1:]:
                t, w, l, r = thread_of(i, nt)
                if t == t0:
                    seen[nt].add("same thread, same round" if r == r0 else "same thread, later round")
                elif w == w0:
                    seen[nt].add("same wave, lower lane" if l < l0 else "same wave, higher lane")
                else:
                    seen[nt].add("lower wave" if w < w0 else "higher wave")
                if abs(t - t0) == 1 and w != w0:
                    seen[nt].add("across a wave boundary")
    want = {"same thread, same round", "same thread, later round", "same wave, lower lane", "same wave, higher lane", "lower wave",
            "higher wave", "across a wave boundary"}
    for nt in PR.NTS:
        assert seen[nt] == want, (nt, want - seen[nt])


def test_gate_cases_have_the_three_distances():
    for c in by_group("gate"):
        d = float(PR.distances(c["px"], c["py"], c["x"], c["y"])[5])
        kind = c["name"].split("_")[1]
        want = {"on": PR.GATE, "inside": np.nextafter(PR.GATE, 0.0), "outside": np.nextafter(PR.GATE, np.inf)}[kind]
        assert d == want, c["name"]
        assert c["expect"] == (5 if kind == "inside" else 0)
    assert len(by_group("gate")) == 6
    assert np.sqrt(np.nextafter(60.0, 0.0) ** 2 + 80.0 ** 2) == 100.0      # (why the offsets are searched, not assumed)


def test_sqrt_cases_differ_where_they_say():
    for c in by_group("same_sqrt") + by_group("one_ulp"):
        ex, ey = c["x"] - c["px"], c["y"] - c["py"]
        sq = ex * ex + ey * ey
        d = np.sqrt(sq)
        lo, hi = np.flatnonzero(d < PR.GATE)
        if c["group"] == "same_sqrt":
            assert d[lo] == d[hi] and sq[lo] > sq[hi] and c["expect"] == lo
        else:
            assert d[lo] == np.nextafter(d[hi], np.inf) and c["expect"] == hi


def test_stride_cases_separate_the_associations_and_the_size_of_start():
    def indices(c, how):
        s = c["expect"]
        a = c["v_ref"] * c["dt"] / c["resolution"]
        b = c["v_ref"] * (c["dt"] / c["resolution"])
        return [{"ref": int(s + i * a), "assoc": int(s + i * b), "split": s + int(i * a)}[how] for i in range(c["H"])]

    pick = {c["name"]: c for c in by_group("stride")}
    c = pick["stride_v0.7_dt0.1_at0_H30"]
    assert 0.7 * 0.1 / 0.1 == 0.6999999999999998 and indices(c, "ref")[10] == 6 and indices(c, "assoc")[10] == 7
    c = pick["stride_v0.3_dt0.3_at0_H30"]
    assert indices(c, "ref")[10] == 9 and indices(c, "assoc")[10] == 8
    for v, every in (("1", 1), ("1.2", 5)):     # the exact product is an integer at every i (every fifth i): no index below it
        c = pick["stride_v%s_dt0.1_at3_H30" % v]
        assert [indices(c, "ref")[i] for i in range(0, 30, every)] == [3 + round(i * c["v_ref"]) for i in range(0, 30, every)]
    c = pick["stride_v0.8_dt0_at3_H9"]
    assert indices(c, "ref") == [3] * 9
    c = pick["stride_v0.7_dt0.1_at1000_H30"]
    assert indices(c, "ref")[10] == 1007 and indices(c, "split")[10] == 1006


def test_path_end_cases_run_past_the_end():
    for c in by_group("end"):
        idx, xr, yr, (s0, s1) = window(c)
        n = len(c["px"])
        assert xr[-1] == c["px"][-1] and yr[-1] == c["py"][-1], c["name"]
        assert int(idx + (c["H"] - 1) * (c["v_ref"] * c["dt"] / c["resolution"])) >= n, c["name"]
        if n == 1:
            assert np.all(xr == c["px"][0]) and s0 == s1 == 0
    assert {len(c["px"]) - c["expect"] for c in by_group("end") if len(c["px"]) == 40} == {1, 2, 3}


def test_batch_layout_sets_the_traps():
    px, py = layout_arrays()
    off = np.concatenate([[0], np.cumsum(LAYOUT["lengths"])])
    assert LAYOUT["lengths"] == (1, 2, 255, 257, 1025) and LAYOUT["resolution"] == (0.1, 0.05, 0.1, 0.03, 0.1)
    assert LAYOUT["v_ref"] == (0.7, 0.3, 1.0, 1.2, 0.7)
    for b in (1, 2, 3):
        x, y = LAYOUT["poses"][b]
        own = PR.distances(px[off[b]:off[b + 1]], py[off[b]:off[b + 1]], x, y)
        before = PR.distances(px[off[b] - 1:off[b]], py[off[b] - 1:off[b]], x, y)[0]
        after = PR.distances(px[off[b + 1]:off[b + 1] + 1], py[off[b + 1]:off[b + 1] + 1], x, y)[0]
        assert before < own.min() and after < own.min(), b
        assert own.min() == 1.0 and np.argmin(own) == LAYOUT["expect"][b] and np.sum(own == 1.0) == 1
    got = PR.batch_ref(px, py, LAYOUT["lengths"], LAYOUT["poses"], LAYOUT["v_ref"], LAYOUT["dt"], LAYOUT["resolution"], 30)
    assert [g[0] for g in got] == LAYOUT["expect"]


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("name", PR.MUTATIONS)
def test_every_mutation_is_caught_by_a_case(name):
    """A wrong version no case tells apart from the restatement means the list is too weak."""
    if name in PR.BATCH_MUTATIONS:
        px, py = layout_arrays()
        args = (px, py, LAYOUT["lengths"], LAYOUT["poses"], LAYOUT["v_ref"], LAYOUT["dt"], LAYOUT["resolution"])
        caught = [H for H in (9, 30) if not all(same(a, b) for a, b in zip(PR.batch_ref(*args, H), PR.mutated_batch(name, *args, H)))]
    else:
        caught = [c["name"] for c in CASES if not same(window(c), window(c, lambda *a: PR.mutated(name, *a)))]
    assert caught, name


def test_an_unmutated_name_changes_nothing():
    for c in CASES[::7]:
        assert same(window(c), window(c, lambda *a: PR.mutated("none", *a)))

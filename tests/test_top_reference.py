"""CPU tests of tests/top_reference.py, the checker of ccv_mppi_read_top_candidates' order: its key against numpy's own order of
doubles (np.lexsort((arange(K), -w)), with the NaNs moved to the front in index order), the kernel layout against the order, and
the five mutations, each of which the probe inputs of tests/top_cases.py must tell from the real order at every K that can
carry the difference (K >= 2: one sample has one order).  `python tests/test_top_reference.py` prints DESIGN.md's table."""
import numpy as np

import top_cases as Cs
import top_reference as R

MUTATIONS = ("ties_high", "nan_by_pattern", "nan_last", "ignore_low_byte", "equal_from_high")
# the input on which each mutation must show at every K >= 2 (others may show it too: the table counts them)
SHOWS_ON = {"ties_high": "all_equal", "nan_by_pattern": "nan_mix", "nan_last": "nan_mix", "ignore_low_byte": "subnormal",
            "equal_from_high": "two_values_random"}


def _numpy_top(w, n):
    nan = np.flatnonzero(np.isnan(w))
    rest = np.lexsort((np.arange(w.size), -w))       # (numpy sorts NaN last)
    return np.concatenate([nan, rest[:w.size - nan.size]])[:n]


def test_the_reference_is_numpys_order_with_the_nans_in_front():
    for K in Cs.KS:
        for name, N, vecs in Cs.all_inputs(K):
            for w in vecs:
                idx, wbits = R.top(w, N)
                np.testing.assert_array_equal(idx, _numpy_top(w, N), err_msg="%s K=%d N=%d" % (name, K, N))
                np.testing.assert_array_equal(wbits, R.bits(w)[idx])
                k = R.key(w)[idx]
                assert np.all(k[1:] <= k[:-1])
    rng = np.random.default_rng(5)
    w = np.abs(rng.standard_normal(3000)) * 10.0 ** rng.integers(-300, 300, size=3000)
    np.testing.assert_array_equal(R.order(w), np.lexsort((np.arange(w.size), -w)))


def test_the_key_of_every_nan_is_all_ones_and_of_a_number_its_bits():
    nans = np.concatenate([Cs.NAN_PATTERNS, np.array([0x7FFFFFFFFFFFFFFF, 0x7FF8000000ABCDEF], dtype=np.uint64)]).view(np.float64)
    assert np.all(R.key(nans) == np.uint64(0xFFFFFFFFFFFFFFFF))
    numbers = np.array([0.0, 5e-324, np.finfo(np.float64).tiny, 1.0, 1e308, np.inf])
    k = R.key(numbers)
    np.testing.assert_array_equal(k, R.bits(numbers))
    assert np.all(k[1:] > k[:-1]) and k[-1] < np.uint64(0xFFFFFFFFFFFFFFFF)


def test_the_kernel_layout_is_the_selection_in_index_order():
    """greater-than-T in index order, then the lowest-index equal-to-T in index order; ordering those pairs by (key, index) gives
    top() -- the host's half of the call"""
    for K in Cs.KS:
        for name, N, vecs in Cs.all_inputs(K):
            for w in vecs:
                idx, wbits = R.kernel_layout(w, N)
                k = R.key(w)
                t = np.sort(k)[::-1][N - 1]
                n_greater = int(np.sum(k > t))
                assert np.all(k[idx[:n_greater]] > t) and np.all(k[idx[n_greater:]] == t)
                assert np.all(np.diff(idx[:n_greater]) > 0) and np.all(np.diff(idx[n_greater:]) > 0)
                np.testing.assert_array_equal(idx[n_greater:], np.flatnonzero(k == t)[:N - n_greater])
                np.testing.assert_array_equal(wbits, R.bits(w)[idx])
                want, _ = R.top(w, N)
                np.testing.assert_array_equal(idx[np.lexsort((idx, ~k[idx]))], want, err_msg="%s K=%d N=%d" % (name, K, N))


def _differs(w, N, mutation):
    """(the ordered result differs, the kernel layout differs) under one mutation"""
    kw = {mutation: True}
    return (not np.array_equal(R.top(w, N)[0], R.top(w, N, **kw)[0]),
            not np.array_equal(R.kernel_layout(w, N)[0], R.kernel_layout(w, N, **kw)[0]))


def mutation_table():
    """{mutation: {input: (launches of three vectors on which the ordered result differs, ... the layout differs, launches)}}"""
    table = {m: {} for m in MUTATIONS}
    for K in Cs.KS:
        for name, N, vecs in Cs.all_inputs(K):
            base = name if not name.startswith("digit") else ("digit0" if name == "digit0" else "digit1-7")
            for m in MUTATIONS:
                d = [_differs(w, N, m) for w in vecs]
                a, b, c = table[m].get(base, (0, 0, 0))
                table[m][base] = (a + any(x for x, _ in d), b + any(y for _, y in d), c + 1)
    return table


def test_every_mutation_shows_on_its_input_at_every_k_from_two():
    for m in MUTATIONS:
        for K in Cs.KS[1:]:
            hits = [(N, _differs(w, N, m)) for name, N, vecs in Cs.all_inputs(K) if name == SHOWS_ON[m] for w in vecs]
            assert any(o for _, (o, _) in hits), (m, K)
            if m != "ties_high":   # (which equal samples are chosen is not the host order's to decide)
                assert any(l for _, (_, l) in hits), (m, K)
    # ... and at the very first place, what a caller of count = 1 sees
    a, b = Cs.NAN_PATTERNS[[3, 0]].view(np.float64)
    assert R.top(np.array([a, b]), 1)[0][0] == 0 and R.top(np.array([b, a]), 1, nan_by_pattern=True)[0][0] == 1
    assert R.top(np.array([1.0, np.nan]), 1)[0][0] == 1 and R.top(np.array([1.0, np.nan]), 1, nan_last=True)[0][0] == 0
    assert R.top(np.array([2.0, 2.0]), 1)[0][0] == 0 and R.top(np.array([2.0, 2.0]), 1, ties_high=True)[0][0] == 1
    assert R.top(np.array([2.0, 2.0]), 1, equal_from_high=True)[0][0] == 1
    assert R.top(np.array([5e-324, 1e-323]), 1)[0][0] == 1 and R.top(np.array([5e-324, 1e-323]), 1, ignore_low_byte=True)[0][0] == 0


def test_one_sample_has_one_order():
    for name, N, vecs in Cs.all_inputs(1):
        for w in vecs:
            for m in MUTATIONS:
                assert _differs(w, N, m) == (False, False)


if __name__ == "__main__":
    t = mutation_table()
    names = sorted({n for m in t.values() for n in m})
    print("| input | launches | " + " | ".join(MUTATIONS) + " |")
    print("| --- | --- | " + " | ".join("---" for _ in MUTATIONS) + " |")
    for n in names:
        print("| %s | %d | " % (n, t[MUTATIONS[0]][n][2]) + " | ".join("%d / %d" % t[m][n][:2] for m in MUTATIONS) + " |")

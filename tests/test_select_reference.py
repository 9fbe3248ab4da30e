"""CPU tests of tests/select_reference.py, the checker of ccv_mppi_batch_read_best_candidates' order: its 64-bit key against
numpy's own order of doubles (np.lexsort((arange(K), cost)): NaN last, -0.0 equal to +0.0, stable in the index), and two
mutations of the order that these inputs must tell from the real one."""
import numpy as np

import select_reference as R


def _bits(*words):
    return np.array(words, dtype=np.uint64).view(np.float64)


TINY = np.finfo(np.float64).tiny
SUB = 5e-324
NANS = _bits(0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0x7FF8000000ABCDEF)
SPECIAL = np.concatenate([[0.0, -0.0, np.inf, -np.inf, SUB, -SUB, TINY, -TINY, 1.0, -1.0, 1.5, -1.5, 1e308, -1e308, 0.0, -0.0, 3.0, 3.0],
                          NANS, [2.0, -np.inf, np.inf, -0.0]])


def _numpy_order(c):
    return np.lexsort((np.arange(c.size), c))


def test_the_key_orders_special_values_as_numpy_does():
    rng = np.random.default_rng(7)
    for trial in range(20):
        c = SPECIAL[rng.permutation(SPECIAL.size)]
        np.testing.assert_array_equal(R.order(c), _numpy_order(c))
        for n in (1, 2, c.size // 2, c.size):
            idx, key = R.lowest(c, n)
            np.testing.assert_array_equal(idx, _numpy_order(c)[:n])
            assert np.all(key[1:] >= key[:-1])


def test_the_key_of_every_nan_is_all_ones_and_of_both_zeros_the_same():
    assert np.all(R.key(NANS) == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert R.key([0.0])[0] == R.key([-0.0])[0] == np.uint64(1 << 63)
    finite = np.array([-np.inf, -1e308, -1.0, -TINY, -SUB, 0.0, SUB, TINY, 1.0, 1e308, np.inf])
    k = R.key(finite)
    assert np.all(k[1:] > k[:-1]) and k[-1] < np.uint64(0xFFFFFFFFFFFFFFFF)


def test_the_key_is_monotone_on_random_bit_patterns():
    rng = np.random.default_rng(11)
    c = rng.integers(0, 2 ** 64, size=4096, dtype=np.uint64).view(np.float64)
    np.testing.assert_array_equal(R.order(c), _numpy_order(c))
    c = rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, size=1000)
    np.testing.assert_array_equal(R.order(c), _numpy_order(c))


def test_all_equal_input_comes_out_by_index():
    for v in (3.25, 0.0, -0.0, np.inf, np.nan):
        np.testing.assert_array_equal(R.order(np.full(100, v)), np.arange(100))
    mixed = np.where(np.arange(64) % 2 == 0, 0.0, -0.0)
    np.testing.assert_array_equal(R.order(mixed), np.arange(64))


def test_the_two_mutations_are_told_from_the_real_order():
    c = SPECIAL.copy()
    want = _numpy_order(c)
    assert not np.array_equal(R.order(c, nan_first=True), want)     # NaN ordered first
    assert not np.array_equal(R.order(c, ties_high=True), want)     # ties to the higher index
    # ... at the very first place too: what a caller of count = 1 would see
    assert R.lowest(np.array([np.nan, 1.0]), 1, nan_first=True)[0][0] == 0 and R.lowest(np.array([np.nan, 1.0]), 1)[0][0] == 1
    assert R.lowest(np.array([2.0, 2.0]), 1, ties_high=True)[0][0] == 1 and R.lowest(np.array([2.0, 2.0]), 1)[0][0] == 0

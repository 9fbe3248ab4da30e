"""The order of ccv_mppi_batch_read_best_candidates in numpy (test helper): the 64-bit key of csrc/mppi_select.h select_key()
and the N lowest samples of a cost vector by (key, sample index).

    every NaN, of any sign or payload  -> 0xFFFFFFFFFFFFFFFF
    -0.0                               -> the key of +0.0
    anything else                      -> bits ^ (sign ? ~0 : 1 << 63)

Unsigned key order is -inf < ... < -0 = +0 < ... < +inf < NaN, so (key, index) ascending is np.lexsort((arange(K), cost)):
numpy sorts NaN last, compares -0.0 equal to +0.0, and lexsort is stable in the index.
"""
import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN = np.uint64(1 << 63)


def key(costs, nan_first=False):
    """uint64 keys of float64 costs.  nan_first: a mutation for the tests of this file's tests (NaN ordered before everything)."""
    c = np.ascontiguousarray(costs, dtype=np.float64)
    bits = c.view(np.uint64)
    k = np.where(bits >> np.uint64(63) != 0, ~bits, bits | SIGN)
    k = np.where(c == 0.0, SIGN, k)
    return np.where(np.isnan(c), np.uint64(0) if nan_first else NAN_KEY, k).astype(np.uint64)


def order(costs, nan_first=False, ties_high=False):
    """every sample index, ascending by (key, index).  ties_high: a mutation (equal keys by descending index)."""
    k = key(costs, nan_first)
    i = np.arange(k.size)
    return np.lexsort((-i if ties_high else i, k)).astype(np.int32)


def lowest(costs, n, **mutation):
    """the n lowest samples of one cost vector: (idx int32 [n], key uint64 [n])"""
    idx = order(costs, **mutation)[:n]
    return idx, key(costs, mutation.get("nan_first", False))[idx]

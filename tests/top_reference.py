"""The order of ccv_mppi_read_top_candidates in numpy (test helper): the 64-bit key of csrc/mppi_top_weights.h top_key(), the N
highest samples of a weight vector by (key descending, sample index ascending), and what top_weights() must leave in its output
buffers before the host puts them in order.

    every NaN, of any sign or payload  -> 0xFFFFFFFFFFFFFFFF
    anything else                      -> its bits

on the domain w >= +0 or NaN (all that exp() produces), where the unsigned order of the bits is the order of the numbers: NaN
weights first, by index among themselves, then +inf, then the finite weights descending, ties to the lower index.

The keyword arguments are MUTATIONS, wrong versions for tests/test_top_reference.py to tell from the real order:
    ties_high         equal keys by descending index
    nan_by_pattern    a NaN's key is its bit pattern (what the kernel and the host sort did before top_key())
    nan_last          NaN ordered behind every number
    ignore_low_byte   the lowest byte of the key ignored (a radix select without its last pass)
    equal_from_high   of the samples equal to the N-th key, the highest-index ones taken
"""
import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW_BYTE = np.uint64(0xFF)


def bits(w):
    return np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)


def key(w, nan_by_pattern=False, nan_last=False, ignore_low_byte=False, **_):
    """uint64 keys of float64 weights (nan_last: NaN gets key 0 and order() ranks it behind the numbers)"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    k = bits(w).copy()
    if ignore_low_byte:
        k &= ~LOW_BYTE
    if not nan_by_pattern:
        k[np.isnan(w)] = np.uint64(0) if nan_last else NAN_KEY
    return k


def _classes(w, **mutation):
    """(rank int64 [K], the higher the earlier): samples of equal rank are ties.  Dense ranks of (not-NaN-last, key)."""
    k = key(w, **mutation)
    behind = np.zeros(k.size, dtype=bool)
    if mutation.get("nan_last") and not mutation.get("nan_by_pattern"):
        behind = np.isnan(np.asarray(w, dtype=np.float64))
    order = np.lexsort((k, ~behind))                     # ascending: the NaNs of nan_last before everything, then by key
    ks, bs = k[order], behind[order]
    step = np.concatenate([[0], ((ks[1:] != ks[:-1]) | (bs[1:] != bs[:-1])).astype(np.int64)])
    rank = np.empty(k.size, dtype=np.int64)
    rank[order] = np.cumsum(step)
    return rank


def order(w, **mutation):
    """every sample index, by (key descending, index ascending)"""
    rank = _classes(w, **mutation)
    i = np.arange(rank.size)
    return np.lexsort((-i if mutation.get("ties_high") else i, -rank)).astype(np.int32)


def kernel_layout(w, n, **mutation):
    """what top_weights() must write: (idx int32 [n], weight bits uint64 [n]) -- all samples with key > T in index order, then the
    lowest-index n_equal samples with key == T in index order, T the n-th highest key"""
    rank = _classes(w, **mutation)
    t = np.sort(rank)[::-1][n - 1]
    greater = np.flatnonzero(rank > t)
    equal = np.flatnonzero(rank == t)
    n_equal = n - greater.size
    assert 1 <= n_equal <= equal.size
    equal = equal[equal.size - n_equal:] if mutation.get("equal_from_high") else equal[:n_equal]
    idx = np.concatenate([greater, equal]).astype(np.int32)
    return idx, bits(w)[idx]


def top(w, n, **mutation):
    """the n highest samples of one weight vector, in order: (idx int32 [n], weight bits uint64 [n])"""
    if mutation.get("equal_from_high"):   # (the selection is the kernel's; the order of the selected is the real one)
        sel, _ = kernel_layout(w, n, **mutation)
        rank = _classes(w, **mutation)[sel]
        idx = sel[np.lexsort((sel, -rank))]
    else:
        idx = order(w, **mutation)[:n]
    return idx.astype(np.int32), bits(w)[idx]

"""The inputs of the top-candidates probe (test helper): weight vectors on the domain w >= +0 or NaN, made
the same way for tests/test_top_reference.py (CPU: every mutation of tests/top_reference.py must show on them) and for
tests/test_gpu_top_candidates.py (the device).  Every input is three vectors of K doubles; those that depend on the count N are
made per N."""
import numpy as np

KS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
NAN_PATTERNS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
LOW, HIGH = 0.25, 0.75           # the two values of the two-valued inputs
BLOCKS = (64, 1024, 2048)        # a wave; the compaction's block (kTopBlock); its second block


def counts_for(K):
    return sorted({n for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, K - 1, K) if 1 <= n <= K})


def one_byte_varies(K, digit, seg):
    """non-negative doubles whose keys differ in radix digit `digit` only (K > 256: in runs of equal values); no NaN, no inf"""
    words = np.full(K, 0x4010203040506070, dtype=np.uint64) & ~np.uint64(0xFF << (8 * digit))
    byte = (np.arange(K, dtype=np.uint64) * np.uint64(7 + 2 * seg)) & np.uint64(0x7F if digit == 7 else 0xFF)
    return (words | (byte << np.uint64(8 * digit))).view(np.float64)


def run_across(K, N, block, s):
    """HIGH, then a contiguous run of LOW across index block - 1 | block, then HIGH again, the N-th place inside the run.  Where
    N > block the last selected LOW sample is index block - 1 + s (s = 0: the cut is the boundary itself), so the selected part of
    the run lies on both sides; otherwise the run starts at N - 1 - s and the cut comes before the boundary.  None if K <= block."""
    if K <= block:
        return None
    if N > block:
        last = min(block - 1 + s, N - 1)
        after = N - 1 - last                  # HIGH samples behind the run
        start = min(block - 2, last)
    else:
        after, start = 0, max(0, N - 1 - s)
    w = np.full(K, HIGH)
    w[start:K - after] = LOW
    n_high = start + after
    assert n_high < N <= n_high + (K - after - start) and start < block <= K - after   # (the run ends AT the boundary only where N = K)
    return w


def fixed_inputs(K, rng):
    """{name: [3 vectors]} that do not depend on N"""
    out = {"random": [np.exp(-rng.uniform(0.0, 12.0 * np.log(10.0), size=K)) for _ in range(3)],
           "all_equal": [np.full(K, v) for v in (1.0, np.inf, 0.0)],
           "zero_but_few": [], "subnormal": [], "nan_mix": []}
    for s in range(3):
        w = np.zeros(K)
        few = rng.permutation(K)[:min(K, 1 + 2 * s)]
        w[few] = rng.uniform(0.1, 1.0, size=few.size)
        out["zero_but_few"].append(w)
        out["subnormal"].append((((np.arange(K) * (7 + 2 * s) + s) & 0xFF) * 5e-324))
    for digit in range(8):   # (digit 0: the lowest byte, the last radix pass; digit 7: the highest, the exponent's top bits)
        out["digit%d" % digit] = [one_byte_varies(K, digit, s) for s in range(3)]
    # finite values, +inf and NaNs of four patterns at shuffled indices.  Forced, so that every K >= 2 carries the differences:
    # vector 0: two NaNs, the lower pattern at the lower index; vector 1: a number before a NaN; vector 2 (K >= 4): both
    pool = np.concatenate([NAN_PATTERNS.view(np.float64), [np.inf, np.inf], rng.uniform(0.0, 2.0, size=10)])
    for s in range(3):
        w = pool[rng.integers(0, pool.size, size=K)].copy()
        spots, wb = np.sort(rng.permutation(K)[:4]), w.view(np.uint64)   # (patterns are written as words: no NaN passes through a float)
        if K >= 2 and s in (0, 2):
            wb[spots[0]], wb[spots[1]] = NAN_PATTERNS[0], NAN_PATTERNS[3]
        if K >= 2 and s == 1:
            w[spots[0]], wb[spots[1]] = 0.5, NAN_PATTERNS[1]
        if K >= 4 and s == 2:
            w[spots[2]], wb[spots[3]] = 1.5, NAN_PATTERNS[2]
        out["nan_mix"].append(w)
    return out


def counted_inputs(K, N, rng):
    """{name: [3 vectors]} with the N-th place inside the run of the lower of two values: N // 2 HIGH ones at random places; the
    LOW ones as a contiguous run across 63|64, across 1023|1024 and across 2047|2048 (where K reaches that far)"""
    out = {"two_values_random": []}
    for s in range(3):
        w = np.full(K, LOW)
        w[rng.permutation(K)[:N // 2]] = HIGH
        out["two_values_random"].append(w)
    for block in BLOCKS:
        runs = [run_across(K, N, block, s) for s in range(3)]
        if runs[0] is not None:
            out["two_values_across_%d" % block] = runs
    return out


def all_inputs(K):
    """[(name, N, [3 vectors])]: every input at every count, from one generator per K"""
    rng = np.random.default_rng(1400 + K)
    fixed = fixed_inputs(K, rng)
    out = []
    for N in counts_for(K):
        out += [(name, N, vecs) for name, vecs in fixed.items()]
        out += [(name, N, vecs) for name, vecs in counted_inputs(K, N, rng).items()]
    return out

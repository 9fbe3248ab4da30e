"""The exact Box-Muller transform of the noise spec, a Philox4x32-10 of its own, and the word sets of the noise tests
(test helper, CPU only; the conventions of update_reference.py and rollout_reference.py).  Nothing here calls the oracle or
the product: oracle/philox_normal.h and csrc/noise_spec.h are the two subjects.

The transform, as a real-number function of two 32-bit words a, b:

    u1 = max(a, 1) / 2^32                       r = sqrt(-2 ln u1)
    theta = (pi/2) (q + g),  q = b >> 30,  g = ((b mod 2^30) - 2^29) / 2^30 in [-1/2, 1/2)
    z0 = r cos theta,  z1 = r sin theta

exact_pair(a, b) -> (r, z0, z1) evaluates it in numpy.longdouble where that has a 64-bit significand (x87):
  -ln u1 = 32 ln 2 - ln a for a < 2^31, and -log1p(-(2^32 - a) / 2^32) for a >= 2^31 (the argument is exact, so nothing is
  lost as u1 -> 1); cos and sin of alpha = (pi/2) g, |alpha| <= pi/4, and the quadrant applied by exchange and sign, which
  is exact.  Rounding, with e = 2^-64 (half an ulp of a 64-bit significand) and libm's logl / log1pl / sinl / cosl / sqrtl
  within one ulp (2 e):
    a < 2^31:  |ln a| <= 21.5 and 32 ln 2 = 22.2 are each off by <= 2 e of themselves, the difference rounds once more; the
               result is >= ln 2, so -ln u1 is off by <= (2 * 21.5 + 2 * 22.2 + 22.2) e / ln 2 < 160 e relative;
    a >= 2^31: 2 e;     the square root halves it and adds 2 e:    r within 82 e;
    alpha: pi/2 (hi + lo doubles, summed) e, the product e; sin, cos 2 e + the argument's 2 e (|alpha| <= pi/4: tan alpha
           <= 1); the product with r e:    z within (82 + 7) e < 2^-57 relative, and |z| <= r.
  An fp32 ulp of r is >= 2^-24 r, so r, z0, z1 are within REF_ULPS = 2^-57 * 2^24 = 2^-33 of an ulp32(r) of the truth;
  test_noise_reference.py pins the longdouble form against exact_pair_mp (mpmath, 200 bits) to that figure.
Where longdouble is narrower, exact_pair evaluates exact_pair_mp word by word and check_pairs thins what it is given
(every THIN-th pair and the zero-angle pairs), as rollout_reference.py does.

check_pairs(a, b, z0, z1) -> (R, Z) in units of ulp32(r_exact), the spacing of floats at the exact radius:
  R = max |z0 - r| over the pairs with b = 2^29 (angle exactly 0: z0 is the radius), Z = max over all pairs and both outputs;
  it asserts that every output is finite, that the radius is positive (z0 > 0 at b = 2^29, z0^2 + z1^2 > 0 everywhere) and
  that each output's sign bit is the exact value's wherever that is not 0.

R_MAX, Z_MAX, R_U1_MAX, Z_U1_MAX: the oracle's figures over PAIRS (the oracle is deterministic: a pin, not a tolerance),
the measured maximum rounded up to the next quarter ulp; the *_U1 pair is the same restricted to a >= 2^32 - 2^16, which is
the "full relative precision as u1 -> 1" of the headers.  The device equals the oracle bit for bit (test_gpu_noise.py).
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
HAVE_LD64 = np.finfo(LD).nmant >= 63
THIN = 257
REF_ULPS = 2.0 ** -33

# measured over PAIRS (tests/test_noise_reference.py prints them): R 1.6335 (a = 0xea314349), Z 2.5126 (a = 0xb8b8669c,
# b = 0x823bab8e); a >= 2^32 - 2^16: R 1.4240, Z 2.0231
R_MAX, Z_MAX = 1.75, 2.75
R_U1_MAX, Z_U1_MAX = 1.5, 2.25

M32 = 0xFFFFFFFF
FOLD = 0xB504F333          # floor(sqrt(2) 2^31): the mantissa word above which the spec folds to [sqrt(1/2), 1)
ZERO_ANGLE = 1 << 29
U1_EDGE = 2 ** 32 - 2 ** 16

_PI_HI, _PI_LO = 3.141592653589793, 1.2246467991473532e-16      # pi = hi + lo to 2^-106


def ulp32(x):
    """the spacing of float32 at |x| (normal range), as float64"""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


# ---- the exact transform ----------------------------------------------------------------------------------------------
def _exact_pair_ld(a, b):
    a = np.maximum(np.asarray(a, dtype=np.uint64), 1)
    b = np.asarray(b, dtype=np.uint64)
    upper = a >= (1 << 31)
    ln2 = np.log(LD(2))
    lo = LD(32) * ln2 - np.log(np.where(upper, 1, a).astype(LD))
    hi = -np.log1p(-((1 << 32) - np.where(upper, a, 1 << 32).astype(np.int64)).astype(LD) / LD(2.0 ** 32))
    r = np.sqrt(LD(2) * np.where(upper, hi, lo))
    f = (b & 0x3FFFFFFF).astype(np.int64) - (1 << 29)
    half_pi = (LD(_PI_HI) + LD(_PI_LO)) / LD(2)
    al = half_pi * (f.astype(LD) / LD(2.0 ** 30))
    c, s = np.cos(al), np.sin(al)
    q = (b >> 30).astype(np.int64)
    cq = np.choose(q, [c, -s, -c, s])
    sq = np.choose(q, [s, c, -s, -c])
    return r, r * cq, r * sq


def exact_pair_mp(a, b, prec=200):
    """(r, z0, z1) of one word pair as mpmath numbers at `prec` >= 160 bits: the definition, nothing clever"""
    import mpmath
    assert prec >= 160
    with mpmath.workprec(prec):
        u1 = mpmath.mpf(max(int(a), 1)) / mpmath.mpf(2) ** 32
        r = mpmath.sqrt(-2 * mpmath.log(u1))
        q, g = int(b) >> 30, mpmath.mpf((int(b) & 0x3FFFFFFF) - (1 << 29)) / mpmath.mpf(2) ** 30
        th = (mpmath.pi / 2) * (q + g)
        # (an exact zero where the angle is a multiple of pi/2: g = 0)
        c = mpmath.cos(th) if (g != 0 or q % 2 == 0) else mpmath.mpf(0)
        s = mpmath.sin(th) if (g != 0 or q % 2 == 1) else mpmath.mpf(0)
        return +r, r * c, r * s


def _mp_to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def exact_pair(a, b):
    """(r, z0, z1), longdouble arrays (module docstring)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.uint64)), np.atleast_1d(np.asarray(b, dtype=np.uint64))
    if HAVE_LD64:
        return _exact_pair_ld(a, b)
    import mpmath
    out = [np.zeros(a.size, dtype=LD) for _ in range(3)]
    with mpmath.workprec(200):
        for i in range(a.size):
            for o, v in zip(out, exact_pair_mp(a[i], b[i])):
                o[i] = _mp_to_ld(v)
    return tuple(out)


_MEMO = {}


def exact_pairs_of_PAIRS():
    """exact_pair over all of PAIRS, computed once per process: (the indices it covers, r, z0, z1)"""
    if "pairs" not in _MEMO:
        a, b = pairs()
        _MEMO["pairs"] = _thinned_exact(a, b)
    return _MEMO["pairs"]


def _thin_index(a, b):
    if HAVE_LD64:
        return np.arange(a.size)
    zero = np.flatnonzero(b == ZERO_ANGLE)
    return np.unique(np.concatenate([np.arange(0, a.size, THIN), zero[::max(1, zero.size // 256)]]))


def _thinned_exact(a, b):
    idx = _thin_index(a, b)
    return (idx,) + exact_pair(a[idx], b[idx])


def check_pairs(a, b, z0, z1, exact=None):
    """(R, Z) of the outputs z0, z1 (float32) at the words a, b (module docstring); `exact`: exact_pairs_of_PAIRS() when
    a, b are PAIRS, so that the reference is computed once"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    z0, z1 = np.asarray(z0, dtype=np.float32), np.asarray(z1, dtype=np.float32)
    assert a.shape == b.shape == z0.shape == z1.shape
    assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1)), "a non-finite normal"
    idx, r, x0, x1 = exact if exact is not None else _thinned_exact(a, b)
    a, b, z0, z1 = a[idx], b[idx], z0[idx], z1[idx]
    assert np.all(z0.astype(np.float64) ** 2 + z1.astype(np.float64) ** 2 > 0.0), "a radius of zero"
    for z, x, name in ((z0, x0, "z0"), (z1, x1, "z1")):
        bad = (x != 0) & (np.signbit(z) != (x < 0))
        assert not bad.any(), "%s has the wrong sign at a = %#x, b = %#x" % (name, a[bad][0], b[bad][0])
    u = ulp32(r.astype(np.float64))
    e0 = np.abs(z0.astype(LD) - x0).astype(np.float64) / u
    e1 = np.abs(z1.astype(LD) - x1).astype(np.float64) / u
    zero = b == ZERO_ANGLE
    assert zero.any(), "no pair with a zero angle: the radius cannot be read"
    assert np.all(z0[zero] > 0)
    R = float(np.max(np.abs(z0[zero].astype(LD) - r[zero]).astype(np.float64) / u[zero]))
    return R, float(max(np.max(e0), np.max(e1)))


def quarter_up(x):
    return math.ceil(x * 4.0) / 4.0


# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, section 3.3) ------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # the two multipliers of the 4x32 round
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # the Weyl increments of the key: golden ratio, sqrt(3) - 1
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]          # Random123 kat_vectors, philox4x32 10 rounds


def philox4x32_10(ctr, key):
    """counters [n][4], key [2] or [n][2] (uint32 values) -> [n][4] uint32; uint64 arithmetic, products < 2^64"""
    x = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4).copy()
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64).reshape(-1, 2), (x.shape[0], 2)).copy()
    mask = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * x[:, 0], np.uint64(PHILOX_M1) * x[:, 2]
        x = np.stack([(p1 >> np.uint64(32)) ^ x[:, 1] ^ k[:, 0], p1 & mask, (p0 >> np.uint64(32)) ^ x[:, 3] ^ k[:, 1], p0 & mask],
                     axis=1)
        k = (k + np.array([PHILOX_W0, PHILOX_W1], dtype=np.uint64)) & mask
    return x.astype(np.uint32)


# ---- the word sets ------------------------------------------------------------------------------------------------------------
SEED = 20261017
N_RANDOM = 1 << 20
# of the random parts, what PAIRS takes (the edges are taken whole): 2^15 random a x 16 + 2^15 random b x 7 + 2^19 pairs
N_RANDOM_IN_PAIRS, N_RANDOM_PAIRS = 1 << 15, 1 << 19


def _rng(tag):
    return np.random.default_rng([SEED, tag])


def _words(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64)


def a_subsets():
    """name -> uint64 words: the parts of A_EDGES"""
    if "a" not in _MEMO:
        j = np.arange(1, 32, dtype=np.uint64)
        p2 = np.uint64(1) << j
        seam = []
        for lz in range(32):
            c = FOLD >> lz                       # a << lz crosses FOLD between c and c + 1
            seam.append(np.arange(max(c - 64, 0), c + 65, dtype=np.uint64))
        _MEMO["a"] = {"tail": np.arange(0, 1 << 16, dtype=np.uint64),
                      "u_to_1": np.arange(U1_EDGE, 1 << 32, dtype=np.uint64),
                      "pow2": np.unique(np.concatenate([p2 - np.uint64(1), p2, p2 + np.uint64(1)])),
                      "fold_seam": np.unique(np.concatenate(seam)),
                      "random": _words(_rng(1), N_RANDOM)}
    return _MEMO["a"]


def b_subsets():
    """name -> uint64 words: the parts of B_EDGES"""
    if "b" not in _MEMO:
        d = np.arange(-4096, 4097, dtype=np.int64)
        seams = [(q * (1 << 30) + h + d) % (1 << 32) for q in range(4) for h in (0, 1 << 29)]
        _MEMO["b"] = {"seams": np.concatenate(seams).astype(np.uint64), "random": _words(_rng(2), N_RANDOM)}
    return _MEMO["b"]


def A_EDGES():
    return np.concatenate(list(a_subsets().values()))


def B_EDGES():
    return np.concatenate(list(b_subsets().values()))


def b16():
    """16 angle words, two per quadrant and half: a random one; and the zero angle q 2^30 + 2^29 (upper half), the seam
    q 2^30 (lower half, alpha = -pi/4).  b = 2^29 is where check_pairs reads the radius."""
    rng = _rng(3)
    out = []
    for q in range(4):
        lo, hi = rng.integers(1, 1 << 29, size=2)
        out += [q << 30, (q << 30) + int(lo), (q << 30) + ZERO_ANGLE, (q << 30) + ZERO_ANGLE + int(hi)]
    return np.array(out, dtype=np.uint64)


def a7():
    return np.array([1, 2, 0x80000000, FOLD, FOLD + 1, M32, int(_words(_rng(4), 1)[0])], dtype=np.uint64)


def pair_parts():
    """[(name, a, b)]: the parts of PAIRS in order"""
    if "parts" not in _MEMO:
        A, B = a_subsets(), b_subsets()
        bs, aa = b16(), a7()
        parts = []
        for name, w in A.items():
            w = w[:N_RANDOM_IN_PAIRS] if name == "random" else w
            parts.append(("a_" + name, np.repeat(w, bs.size), np.tile(bs, w.size)))
        for name, w in B.items():
            w = w[:N_RANDOM_IN_PAIRS] if name == "random" else w
            parts.append(("b_" + name, np.tile(aa, w.size), np.repeat(w, aa.size)))
        r = _words(_rng(5), 2 * N_RANDOM_PAIRS)
        parts.append(("random_pairs", r[:N_RANDOM_PAIRS], r[N_RANDOM_PAIRS:]))
        assert sum(p[1].size for p in parts) < 1 << 22
        _MEMO["parts"] = parts
    return _MEMO["parts"]


def pairs():
    """PAIRS: (a, b), uint64 arrays of 32-bit words"""
    if "ab" not in _MEMO:
        parts = pair_parts()
        _MEMO["ab"] = (np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    return _MEMO["ab"]


def sample_of_pairs(per_part=400, tag=6):
    """a few words of every part of PAIRS (seeded), with each part's first and last pair and, of the parts that cross A_EDGES
    with b16, pairs at the zero angle: what the slow forms (mpmath, the rational restatement) are run on"""
    rng = _rng(tag)
    sa, sb = [], []
    for name, a, b in pair_parts():
        idx = np.unique(np.concatenate([[0, a.size - 1], rng.integers(0, a.size, size=per_part)]))
        if name.startswith("a_"):
            zero = np.flatnonzero(b == ZERO_ANGLE)
            idx = np.unique(np.concatenate([idx, zero[:8], zero[-8:], zero[rng.integers(0, zero.size, size=per_part // 8)]]))
        sa.append(a[idx])
        sb.append(b[idx])
    return np.concatenate(sa), np.concatenate(sb)


# ---- the spec restated in exact rational arithmetic, rounded to fp32 after every operation -----------------------------------------
def r32(x):
    """the float32 nearest to the Fraction x (ties to even; normal range, which is all the spec reaches), as a Fraction"""
    if x == 0:
        return Fraction(0)
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1                                    # 2^e <= |x| < 2^(e+1)
    assert e >= -126
    sh = e - 23
    num, den = n << max(-sh, 0), d << max(sh, 0)
    q, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and (q & 1)):
        q += 1
    v = Fraction(q) * (Fraction(2) ** sh)
    return -v if x < 0 else v


def sqrt32(x):
    """the correctly rounded float32 square root of the dyadic Fraction x >= 0"""
    n, d = x.numerator, x.denominator
    assert d & (d - 1) == 0 and n >= 0
    if n == 0:
        return Fraction(0)
    k = 64 + d.bit_length()
    N = (n << (2 * k)) // d
    s = math.isqrt(N)                             # >= 2^40: an integer or s + 1/2 rounds to 24 bits as the root itself does
    return r32(Fraction(2 * s + (0 if s * s == N else 1), 1 << (k + 1)))


def _hexf(s):
    return Fraction(float.fromhex(s))


Q = [_hexf(s) for s in ("0x1.715476p+0", "-0x1.715476p-1", "0x1.ec73e0p-2", "-0x1.715946p-2", "0x1.26cfb8p-2",
                        "-0x1.e9df04p-3", "0x1.ba9caap-3", "-0x1.a548fcp-3", "0x1.f702acp-4")]
S = [_hexf(s) for s in ("-0x1.555556p-3", "0x1.11110ep-7", "-0x1.a013a2p-13", "0x1.6dbc3ep-19")]
C = [_hexf(s) for s in ("-0x1.000000p-1", "0x1.55554cp-5", "-0x1.6c0df8p-10", "0x1.9a6a98p-16")]
TWO_LN2, HALF_PI_30 = _hexf("0x1.62e430p+0"), _hexf("0x1.921fb6p-30")
MUTATIONS = ("t_from_float_m", "zero_not_mapped", "top_term_dropped", "fold_one_binade_down", "angle_not_centred",
             "no_exchange_in_odd_quadrants", "cos_sign_one_quadrant_off", "sin_sign_one_quadrant_off", "ln2_not_2ln2")


def spec_pair(a, b, mutation=None):
    """DESIGN.md section 3 for one word pair -> (z0, z1) as numpy.float32 (with -0.0 where the spec gives it), or one wrong
    version of it"""
    assert mutation is None or mutation in MUTATIONS
    a, b = int(a), int(b)
    a1 = a if (a or mutation == "zero_not_mapped") else 1
    lz = 32 - a1.bit_length()                     # (a word of 0, unmapped: 32 leading zeros, mantissa word 0)
    m = (a1 << lz) & M32
    fold = m > (FOLD >> 1 if mutation == "fold_one_binade_down" else FOLD)
    if mutation == "t_from_float_m":
        t = r32(r32(Fraction(m)) * Fraction(1, 1 << (32 if fold else 31)) - 1)
    elif fold:
        t = -(r32(Fraction((0 - m) & M32)) * Fraction(1, 1 << 32))
    else:
        t = r32(Fraction((m - 0x80000000) & M32)) * Fraction(1, 1 << 31)
    L0 = Fraction(1 + lz - (1 if fold else 0))
    top = 7 if mutation == "top_term_dropped" else 8
    q = Q[top]
    for i in range(top - 1, -1, -1):
        q = r32(q * t + Q[i])
    L = r32(-t * q + L0)
    r = sqrt32(r32(L * (TWO_LN2 / 2 if mutation == "ln2_not_2ln2" else TWO_LN2)))
    f = (b & 0x3FFFFFFF) - (0 if mutation == "angle_not_centred" else 1 << 29)
    al = r32(r32(Fraction(f)) * HALF_PI_30)
    w = r32(al * al)
    s, c = S[3], C[3]
    for i in (2, 1, 0):
        s, c = r32(s * w + S[i]), r32(c * w + C[i])
    sn = r32(r32(al * w) * s + al)
    cs = r32(w * c + 1)
    quad = b >> 30
    odd = bool(quad & 1) and mutation != "no_exchange_in_odd_quadrants"
    ca, sa = (sn, cs) if odd else (cs, sn)
    cneg = ((quad + (0 if mutation == "cos_sign_one_quadrant_off" else 1)) & 2) != 0      # quadrants 1, 2
    sneg = ((quad + (1 if mutation == "sin_sign_one_quadrant_off" else 0)) & 2) != 0      # quadrants 2, 3
    z0, z1 = np.float32(float(r32(r * ca))), np.float32(float(r32(r * sa)))
    return (-z0 if cneg else z0), (-z1 if sneg else z1)


def spec_pairs(a, b, mutation=None):
    out = [spec_pair(x, y, mutation) for x, y in zip(a, b)]
    return np.array([o[0] for o in out], dtype=np.float32), np.array([o[1] for o in out], dtype=np.float32)

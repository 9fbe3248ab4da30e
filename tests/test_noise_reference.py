"""CPU: pins tests/noise_reference.py and holds the oracle's noise spec (oracle/philox_normal.h) to the exact transform.

  * the longdouble form of the exact transform against mpmath at 200 bits, to the bound derived from the 64-bit significand;
  * the numpy Philox against the Random123 vectors and the oracle's Philox;
  * the oracle's normal_pairs over all of PAIRS: R (radius) and Z (z0, z1) in ulp32(r_exact), asserted at the measured
    maximum rounded up to a quarter ulp (noise_reference.R_MAX, Z_MAX), and on its own for a >= 2^32 - 2^16, which is the
    headers' "full relative precision as u1 -> 1";
  * the spec restated in exact rational arithmetic equals the oracle bit for bit, and nine wrong versions of it leave the
    bounds or fail the sign check;
  * the device probe cross-compiles with the product's flags (tests/test_gpu_noise.py runs it).
"""
import os
import subprocess

import numpy as np
import pytest

import noise_probe
import noise_reference as NR
from oracle import oracle_lib as O

LD = np.longdouble


def bits(z):
    return np.asarray(z, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_on_pairs():
    a, b = NR.pairs()
    return (a, b) + O.normal_pairs(a, b)


@pytest.fixture(scope="module")
def slow_sample():
    return NR.sample_of_pairs()


def test_word_sets_hold_what_they_name():
    A, B = NR.a_subsets(), NR.b_subsets()
    assert A["tail"].size == 1 << 16 and A["tail"][0] == 0 and A["tail"][1] == 1
    assert A["u_to_1"].size == 1 << 16 and A["u_to_1"][-1] == NR.M32
    for j in range(1, 32):
        assert all(int(w) in A["pow2"] for w in ((1 << j) - 1, 1 << j, min((1 << j) + 1, NR.M32)))
    for lz in range(32):
        c = NR.FOLD >> lz
        assert all(w in A["fold_seam"] for w in (max(c - 64, 0), c, c + 1, c + 64))
    assert A["random"].size == 1 << 20 and B["random"].size == 1 << 20
    for q in range(4):
        for h in (0, 1 << 29):
            assert all(((q << 30) + h + d) % (1 << 32) in B["seams"] for d in (-4096, -1, 0, 1, 4096))
    b16 = NR.b16()
    assert NR.ZERO_ANGLE in b16 and b16.size == 16
    halves = {(int(w) >> 30, (int(w) & 0x3FFFFFFF) >= (1 << 29)) for w in b16}
    assert len(halves) == 8                                        # every quadrant, both halves
    a, b = NR.pairs()
    assert a.size == b.size < 1 << 22 and a.max() <= NR.M32 and b.max() <= NR.M32
    edges = sum(w.size for n, w in A.items() if n != "random") * 16 + B["seams"].size * 7
    assert a.size - edges >= 1 << 20                               # (the edges are whole; the random parts fill the rest)


def test_ulp32():
    for x, want in ((1.0, 2.0 ** -23), (1.9999, 2.0 ** -23), (2.0, 2.0 ** -22), (0.75, 2.0 ** -24), (6.66, 2.0 ** -21),
                    (2.2e-5, float(np.spacing(np.float32(2.2e-5))))):
        assert NR.ulp32(x) == want
    x = np.abs(np.random.default_rng(3).normal(size=1000)).astype(np.float32) + np.float32(1e-6)
    np.testing.assert_array_equal(NR.ulp32(x), np.spacing(x).astype(np.float64))


def test_longdouble_form_against_mpmath(slow_sample):
    """>= 2000 words from every part of PAIRS; the bound is REF_ULPS = 2^-33 ulp32(r) (noise_reference's docstring: 89 half
    ulps of a 64-bit significand relative, against an fp32 ulp of >= 2^-24 r).  Measured: 2^-37."""
    import mpmath
    a, b = slow_sample
    assert a.size >= 2000
    r, z0, z1 = NR.exact_pair(a, b)
    worst = 0.0
    with mpmath.workprec(200):
        for i in range(a.size):
            want = NR.exact_pair_mp(a[i], b[i])
            u = mpmath.mpf(float(NR.ulp32(float(want[0]))))
            for got, w in zip((r[i], z0[i], z1[i]), want):
                hi = float(got)
                g = mpmath.mpf(hi) + mpmath.mpf(float(got - LD(hi)))
                worst = max(worst, float(abs(g - w) / u))
                assert (w == 0) == (got == 0)
    print("longdouble against mpmath: 2^%.1f ulp32(r)" % np.log2(worst))
    assert worst <= NR.REF_ULPS


def test_mpmath_form_at_known_points():
    import mpmath
    with mpmath.workprec(200):
        r, z0, z1 = NR.exact_pair_mp(0, NR.ZERO_ANGLE)              # a = 0 is a = 1: r = sqrt(64 ln 2), angle 0
        assert abs(r - mpmath.sqrt(64 * mpmath.log(2))) < mpmath.mpf(2) ** -190 and z0 == r and z1 == 0
        r, z0, z1 = NR.exact_pair_mp(1 << 31, (1 << 30) + NR.ZERO_ANGLE)     # u1 = 1/2, angle pi/2
        assert abs(r - mpmath.sqrt(2 * mpmath.log(2))) < mpmath.mpf(2) ** -190 and z0 == 0 and z1 == r
        r, z0, z1 = NR.exact_pair_mp(NR.M32, 3 << 30)               # angle 3 pi/2 - pi/4: both negative, equal
        assert z0 < 0 and z1 < 0 and abs(z0 - z1) < mpmath.mpf(2) ** -190
        assert abs(r * r - 2 ** -31) < mpmath.mpf(2) ** -62         # -2 ln(1 - 2^-32) = 2^-31 (1 + 2^-33 + ...)


def test_numpy_philox_known_answers_and_the_oracle():
    for ctr, key, want in NR.KAT:
        assert NR.philox4x32_10([ctr], key)[0].tolist() == list(want)
        assert O.philox_blocks([ctr], key)[0].tolist() == list(want)
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(100000, 4), dtype=np.uint64)
    ones = np.array([[0, 0, 0, 0], [NR.M32] * 4, [0, NR.M32, 0, NR.M32], [NR.M32, 0, NR.M32, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
    ctr = np.concatenate([ones.astype(np.uint64), ctr])
    keys = [(0, 0), (NR.M32, NR.M32), (0, NR.M32), (NR.M32, 0)] + [tuple(int(v) for v in k) for k in
                                                                    rng.integers(0, 1 << 32, size=(4, 2), dtype=np.uint64)]
    for key in keys:
        np.testing.assert_array_equal(NR.philox4x32_10(ctr, key), O.philox_blocks(ctr, key), err_msg=str(key))
    # a key per counter, as the scalar binding takes it
    kk = rng.integers(0, 1 << 32, size=(64, 2), dtype=np.uint64)
    got = NR.philox4x32_10(ctr[:64], kk)
    for i in range(64):
        assert got[i].tolist() == O.philox4x32_10([int(v) for v in ctr[i]], [int(v) for v in kk[i]])


def test_bulk_bindings_are_the_scalar_ones(slow_sample):
    a, b = slow_sample[0][:300], slow_sample[1][:300]
    z0, z1 = O.normal_pairs(a, b)
    for i in range(a.size):
        s0, s1 = O.normal_pair(int(a[i]), int(b[i]))
        assert bits(s0) == bits(z0[i]) and bits(s1) == bits(z1[i])
    x = O.radius_args(a)
    np.testing.assert_array_equal(bits(np.sqrt(x)), bits(O.normal_pairs(a, np.full(a.size, NR.ZERO_ANGLE))[0]))


def test_oracle_against_the_exact_transform(oracle_on_pairs):
    """R and Z over all of PAIRS.  Measured: R = 1.6335, Z = 2.5126 ulp32(r_exact); asserted: 1.75, 2.75."""
    a, b, z0, z1 = oracle_on_pairs
    R, Z = NR.check_pairs(a, b, z0, z1, NR.exact_pairs_of_PAIRS())
    print("oracle over PAIRS: R = %.4f, Z = %.4f ulp32(r)" % (R, Z))
    assert R <= NR.R_MAX and Z <= NR.Z_MAX
    if NR.HAVE_LD64:                                 # the pin: the constants are the measured maxima rounded up, not more
        assert NR.quarter_up(R) == NR.R_MAX and NR.quarter_up(Z) == NR.Z_MAX


def test_full_relative_precision_as_u1_tends_to_1(oracle_on_pairs):
    """The headers' claim, as a number: over a >= 2^32 - 2^16 (radii from 2.2e-5 to 5.5e-3), R = 1.4240 and Z = 2.0231
    ulp32(r_exact) measured; asserted: 1.5, 2.25.  (An absolute tolerance of 4e-6 is 20 % of the smallest of these radii.)"""
    a, b, z0, z1 = oracle_on_pairs
    idx, r, x0, x1 = NR.exact_pairs_of_PAIRS()
    sel = a[idx] >= NR.U1_EDGE
    assert np.count_nonzero(sel) >= ((1 << 16) * 16 if NR.HAVE_LD64 else 64)
    full = idx[sel]
    R, Z = NR.check_pairs(a[full], b[full], z0[full], z1[full], (np.arange(full.size), r[sel], x0[sel], x1[sel]))
    print("oracle over a >= 2^32 - 2^16: R = %.4f, Z = %.4f ulp32(r)" % (R, Z))
    assert R <= NR.R_U1_MAX and Z <= NR.Z_U1_MAX
    if NR.HAVE_LD64:
        assert NR.quarter_up(R) == NR.R_U1_MAX and NR.quarter_up(Z) == NR.Z_U1_MAX


def test_rational_restatement_is_the_oracle_bit_for_bit(slow_sample):
    a, b = slow_sample
    z0, z1 = NR.spec_pairs(a, b)
    o0, o1 = O.normal_pairs(a, b)
    np.testing.assert_array_equal(bits(z0), bits(o0))
    np.testing.assert_array_equal(bits(z1), bits(o1))
    R, Z = NR.check_pairs(a, b, z0, z1)
    assert R <= NR.R_MAX and Z <= NR.Z_MAX


@pytest.mark.parametrize("mutation", NR.MUTATIONS)
def test_a_wrong_spec_leaves_the_bounds(slow_sample, mutation):
    """Each mistake, on the sample of PAIRS the restatement is run on: beyond R_MAX or Z_MAX, or refused by the sign check."""
    a, b = slow_sample
    z0, z1 = NR.spec_pairs(a, b, mutation)
    try:
        R, Z = NR.check_pairs(a, b, z0, z1)
    except AssertionError as e:
        print("%s: %s" % (mutation, e))
        return
    print("%s: R = %.3g, Z = %.3g" % (mutation, R, Z))
    assert R > NR.R_MAX or Z > NR.Z_MAX


def test_probe_cross_compiles_with_the_products_flags():
    from ccv_mppi_path_tracker_amd import build
    cmd = noise_probe.command("OUT")
    assert cmd[1:1 + len(build.HIPCC_FLAGS)] == build.HIPCC_FLAGS
    assert cmd[1 + len(build.HIPCC_FLAGS):] == ["-I", build.CSRC, "-shared", "-o", "OUT", noise_probe.SOURCE]
    src = open(noise_probe.SOURCE).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"noise_spec.h"']          # nothing else of the product
    path = noise_probe.build_probe()
    assert os.path.exists(path) and not noise_probe.stale()
    syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    for name in ("probe_philox", "probe_box_muller", "probe_sqrt"):
        assert " T " + name in syms

"""GPU tests (-m gpu): the control noise of csrc/noise_spec.h at the words Philox never hands it, and the production path at
the ends of its counters.  The CPU side (the exact transform, the word sets, the oracle's figures) is pinned by
tests/test_noise_reference.py.

Probe (tests/probe/noise_probe.hip: noise_spec.h behind C entry points, built with the product's flags):
  * philox4x32_10 and philox4x32_10_n<3|4|5> on the Random123 vectors, 10^5 random counters under 8 keys, and counters and keys
    of all-zero and all-one words: bit-equal to the oracle and to the numpy Philox of noise_reference.py;
  * box_muller_f32 and box_muller_f32_n<6|8|10> on all of PAIRS (every a < 2^16, every a >= 2^32 - 2^16, the powers of two, the
    seam of the fold in every binade, the quadrant and +-pi/4 seams of b, the zero angle): bit-equal to the oracle's
    normal_pairs, hence to each other;
  * check_pairs on the device's own output: the oracle's verdict repeated (R <= 1.75, Z <= 2.75 ulp32(r_exact)), so that a
    failure of the bit test still says which side left the exact transform;
  * sqrt_cr_radius against __builtin_sqrtf and numpy's float32 square root on the radius argument of every word of A_EDGES
    and 2^20 floats strided over [2^-40, 2^7] with both ends.  tools/microbench/sqrt_check.hip stays the exhaustive hand-run
    check of that domain; this is a structured sample of it.

Production path, through the C ABI: CCV_MPPI_KERNEL in {unset, v1, pc, r3, r4, solo} x the three models x (K = 130, H = 9),
(K = 65, H = 4: diff drive draws 6 normals, a partial Philox call).  sampling() + read_controls() and the fused iteration +
read_controls() equal the oracle's philox controls bit for bit at seed in {0, 2^64 - 1}, iteration in {0, 2^32 - 1, 2^32,
2^64 - 1}, sample_offset in {0, 2^31 - 1 - K: the largest ccv_mppi_create admits}, with a zero warm start and
  "wide":     sigma = 1, bounds +-1e30: a control is double(z).  Bounds like these leave the range the host admits to the
              cooperative kernels' sin / cos (fast_trig_safe), so the fused iteration runs the plain kernel whatever the family;
  "admitted": sigma = 2^-4, bounds +-0.5: |z| <= 6.66 never reaches them (a control is double(z) / 16 exactly), every turn per
              step stays below pi/4, and the fused iteration runs the family's own kernel with its N-wide noise.
"""
import numpy as np
import pytest

import helpers
import noise_probe as P
import noise_reference as NR
from ccv_mppi_path_tracker_amd import capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController
from oracle import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()
    P.lib()


def bits(z):
    return np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)


# ---- Philox -------------------------------------------------------------------------------------------------------------------
def philox_inputs():
    rng = np.random.default_rng(12)
    ext = [[0, 0, 0, 0], [NR.M32] * 4, [0, NR.M32, 0, NR.M32], [NR.M32, 0, NR.M32, 0], [NR.M32, 0, 0, 0], [0, 0, 0, NR.M32]]
    ctr = np.concatenate([np.array(ext, dtype=np.uint64), rng.integers(0, 1 << 32, size=(100000, 4), dtype=np.uint64)])
    keys = [(0, 0), (NR.M32, NR.M32), (0, NR.M32), (NR.M32, 0)]
    keys += [tuple(int(v) for v in k) for k in rng.integers(0, 1 << 32, size=(4, 2), dtype=np.uint64)]
    return ctr, keys


@pytest.mark.parametrize("form", P.PHILOX_FORMS)
def test_philox_forms_bit_equal(form):
    for ctr, key, want in NR.KAT:
        for n in (1, 7):           # (alone, padded up to N blocks; and over more than one thread of the N-wide form)
            got = P.philox(form, [ctr] * n, key)
            assert got.tolist() == [list(want)] * n, (form, ctr, key)
    ctr, keys = philox_inputs()
    assert len(keys) == 8 and ctr.shape[0] % 3 and ctr.shape[0] % 4 and ctr.shape[0] % 5   # (the last thread's blocks: padding)
    for key in keys:
        got, want = P.philox(form, ctr, key), O.philox_blocks(ctr, key)
        np.testing.assert_array_equal(want, NR.philox4x32_10(ctr, key), err_msg="oracle / numpy, key %s" % (key,))
        np.testing.assert_array_equal(got, want, err_msg="form %d, key %s" % (form, key))


# ---- Box-Muller ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_pairs():
    a, b = NR.pairs()
    return (a, b) + O.normal_pairs(a, b)


_DEVICE = {}


def device_pairs(form):
    if form not in _DEVICE:
        a, b = NR.pairs()
        _DEVICE[form] = P.box_muller(form, a, b)
    return _DEVICE[form]


@pytest.mark.parametrize("form", P.BOX_MULLER_FORMS)
def test_box_muller_forms_bit_equal_on_all_pairs(oracle_pairs, form):
    a, b, o0, o1 = oracle_pairs
    z0, z1 = device_pairs(form)
    diff = (bits(z0) != bits(o0)) | (bits(z1) != bits(o1))
    if diff.any():
        i = int(np.flatnonzero(diff)[0])
        part = [n for n, lo, hi in part_ranges() if lo <= i < hi][0]
        pytest.fail("form %d: %d of %d pairs differ from the oracle; the first: a = %#010x, b = %#010x (%s): device (%r, %r) = "
                    "(%#010x, %#010x), oracle (%r, %r) = (%#010x, %#010x)"
                    % (form, int(diff.sum()), a.size, a[i], b[i], part, z0[i], z1[i], bits(z0)[i], bits(z1)[i], o0[i], o1[i],
                       bits(o0)[i], bits(o1)[i]))


def part_ranges():
    out, lo = [], 0
    for name, a, _ in NR.pair_parts():
        out.append((name, lo, lo + a.size))
        lo += a.size
    return out


@pytest.mark.parametrize("form", P.BOX_MULLER_FORMS)
def test_device_output_against_the_exact_transform(form):
    a, b = NR.pairs()
    z0, z1 = device_pairs(form)
    R, Z = NR.check_pairs(a, b, z0, z1, NR.exact_pairs_of_PAIRS())
    print("device form %d over PAIRS: R = %.4f, Z = %.4f ulp32(r)" % (form, R, Z))
    assert R <= NR.R_MAX and Z <= NR.Z_MAX
    u1 = a >= NR.U1_EDGE
    idx, r, x0, x1 = NR.exact_pairs_of_PAIRS()
    sel = u1[idx]
    full = idx[sel]
    R1, Z1 = NR.check_pairs(a[full], b[full], z0[full], z1[full], (np.arange(full.size), r[sel], x0[sel], x1[sel]))
    print("device form %d over a >= 2^32 - 2^16: R = %.4f, Z = %.4f ulp32(r)" % (form, R1, Z1))
    assert R1 <= NR.R_U1_MAX and Z1 <= NR.Z_U1_MAX


# ---- the radius' square root ----------------------------------------------------------------------------------------------------
def test_sqrt_cr_radius_is_the_correctly_rounded_root():
    lo, hi = int(np.float32(2.0 ** -40).view(np.uint32)), int(np.float32(2.0 ** 7).view(np.uint32))
    strided = np.linspace(lo, hi, 1 << 20).round().astype(np.uint32)
    assert strided[0] == lo and strided[-1] == hi
    x_edges = O.radius_args(NR.A_EDGES())
    assert x_edges.min() >= 2.0 ** -40 and x_edges.max() <= 2.0 ** 7
    x = np.concatenate([x_edges, strided.view(np.float32)])
    s_cr, s_builtin = P.sqrt(x)
    want = np.sqrt(x)
    assert want.dtype == np.float32
    for got, name in ((s_cr, "sqrt_cr_radius"), (s_builtin, "__builtin_sqrtf")):
        bad = bits(got) != bits(want)
        assert not bad.any(), "%s(%r) = %r, the correctly rounded root is %r (%d of %d differ)" % (
            name, x[bad][0], got[bad][0], want[bad][0], int(bad.sum()), x.size)
    np.testing.assert_array_equal(bits(s_cr), bits(s_builtin))


# ---- the production path at the ends of its counters --------------------------------------------------------------------------------
FAMILIES = (None, "v1", "pc", "r3", "r4", "solo")
MODELS = ("diff_drive", "steering_diff_drive", "full_body")
SHAPES = ((130, 9), (65, 4))
SETS = {"wide": (1.0, 1.0e30), "admitted": (2.0 ** -4, 0.5)}
SEEDS = (0, 2 ** 64 - 1)
ITERATIONS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)


def largest_offset(K):
    """the largest sample_offset ccv_mppi_create admits: sample_offset + K <= 2^31 - 1 (ccv_mppi_capi.hip; the refusal of the
    next one is tests/test_abi.py's)"""
    return 2 ** 31 - 1 - K


def params_of(model, K, H, which):
    mk = {"diff_drive": configs.diff_drive_defaults, "steering_diff_drive": configs.steering_defaults,
          "full_body": configs.full_body_defaults}[model]
    sigma, bound = SETS[which]
    p = mk(K, H)
    return p.with_(control_noise=sigma, u_min=(-bound,) * p.udim, u_max=(bound,) * p.udim, dt=0.1)


_ORACLE = {}


def oracle_controls(p, which, seed, it, off):
    key = (p.model, p.num_samples, p.horizon, which, seed, it, off)
    if key not in _ORACLE:
        o = helpers.oracle_for(p)
        o.set_nominal(np.zeros((p.horizon - 1, p.udim)))
        o.sampling(seed, rng="philox", iteration=it, k_offset=off)
        u = o.get_controls()
        if which == "wide":       # a control is double(z): the oracle's own normals, counter by counter
            z = O.normals(seed, it, off, p.num_samples, (p.horizon - 1) * p.udim).astype(np.float64)
            np.testing.assert_array_equal(u, z.reshape(u.shape))
        assert np.all(np.abs(u) < SETS[which][1])                   # (no bound was reached)
        _ORACLE[key] = u
    return _ORACLE[key]


@pytest.mark.parametrize("K,H", SHAPES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("family", FAMILIES)
def test_production_noise_at_the_counter_extremes(monkeypatch, family, model, K, H):
    if family:
        monkeypatch.setenv("CCV_MPPI_KERNEL", family)
    else:
        monkeypatch.delenv("CCV_MPPI_KERNEL", raising=False)
    for which in SETS:
        p = params_of(model, K, H, which)
        zero = np.zeros((H - 1, p.udim))
        state = np.zeros(p.nstate)
        xr, yr = 0.1 * np.arange(H), np.zeros(H)
        for off in (0, largest_offset(K)):
            g = MPPIController(p, sample_offset=off)
            for seed in SEEDS:
                for it in ITERATIONS:
                    want = oracle_controls(p, which, seed, it, off)
                    what = (family, model, K, H, which, off, seed, it)
                    g.set_nominal(zero)
                    g.sampling(seed, it)
                    np.testing.assert_array_equal(g.read_controls(), want, err_msg="sampling %s" % (what,))
                    g.set_nominal(zero)
                    g.iterate(state, p.dt, xr, yr, 0.0, seed, it, want_stats=False)
                    np.testing.assert_array_equal(g.read_controls(), want, err_msg="fused %s" % (what,))
            g.close()

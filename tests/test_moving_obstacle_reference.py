"""Pins tests/moving_obstacle_reference.py: its numpy restatement of the device spec of the moving-disc term (DESIGN.md section
10g), fp64 operation by operation with an exactly rounded fma, lies inside the reference's bounds -- at states within 1e-9 m of
a moving disc's edge, tau at step 127, v = 0, n in {0, 1, 3, 4, 32}, a NaN state -- and seven wrong versions lie outside; with
v = 0 the reference is obstacle_reference's, exactly.  And the CPU side of the interface: the new names declared, exported,
in the ctypes table; the header still C99; a null handle refused; pack_velocities."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moving_obstacle_reference as MR
import obstacle_cases as OC
import obstacle_reference as OR
from ccv_mppi_path_tracker_amd import BatchController, batch, build, capi

LD = np.longdouble
spec = MR.spec
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ccv_mppi.h")
MOVING = {"ccv_mppi_batch_set_obstacle_velocities", "ccv_mppi_batch_get_obstacle_velocities"}


def same_ld(a, b):   # (the bytes of a longdouble include padding)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def scene(n, seed, kmax=14, dt=0.1, still=False):
    """x0, discs [n][3], velocities [n][2], states P [T][2] with their steps ks [T]: random states, the pose at step 0, and for
    the first three discs states within 1e-9 m of the edge and well inside, at the disc's place at the state's own step"""
    rng = np.random.default_rng(seed)
    x0 = np.array([37.25, -12.5]) + rng.uniform(-1, 1, 2)
    discs = np.zeros((n, 3))
    discs[:, :2] = x0 + rng.uniform(-6, 6, (n, 2))
    discs[:, 2] = rng.uniform(0.2, 1.5, n)
    vel = np.zeros((n, 2)) if still else rng.uniform(-1.5, 1.5, (n, 2))
    P, ks = [x0 + rng.uniform(-8, 8, (24, 2)), x0[None, :]], [rng.integers(0, kmax + 1, 24), [0]]
    for j in range(min(n, 3)):
        for k in (kmax, kmax // 2, 1):
            centre = discs[j, :2] + vel[j] * (k * dt)
            P += [OC.ring(rng, centre, discs[j, 2], 4, 1e-9), OC.ring(rng, centre, 0.5 * discs[j, 2], 3, 0.1)]
            ks += [[k] * 4, [k] * 3]
    return x0, discs, vel, np.concatenate(P), np.concatenate(ks).astype(np.int64), dt


# n in {0, 1, 3, 4, 32}; the horizon's usual steps, tau at step 127, v = 0
CASES = [(n, kmax, still) for n in (0, 1, 3, 4, 32) for kmax, still in ((14, False), (127, False), (14, True))]


@pytest.mark.parametrize("n,kmax,still", CASES)
def test_spec_inside_the_bounds(n, kmax, still):
    x0, discs, vel, P, ks, dt = scene(n, 200 + n, kmax, still=still)
    w = 7.5
    s, cost = spec(P, ks, x0, dt, discs, vel, w)
    ref_s = MR.power(P, ks, dt, discs, vel)
    if n == 0:
        assert np.all(np.isinf(ref_s)) and cost == 0.0 and np.all(MR.penalty(P, ks, dt, discs, vel, w) == 0)
        return
    err = np.abs(s.astype(LD) - ref_s).astype(np.float64)
    bnd = MR.bound_s(P, x0, ks, dt, discs, vel)
    print("n=%d kmax=%d still=%s  max err/bound of s: %.3g" % (n, kmax, still, float(np.max(err / bnd))))
    assert np.all(err <= bnd)
    # the conditions: some states penetrate, some lie within 1e-9 m of a moving disc's edge on either side, the last step is there
    assert 4 <= np.count_nonzero(ref_s < 0) < len(P)
    assert np.count_nonzero(np.abs(ref_s) < 1e-8) >= 4
    assert ks.max() == kmax
    tot, tb = MR.sample_penalty(P[None], x0, ks, dt, discs, vel, w)
    assert abs(LD(cost) - tot[0]) <= tb[0], (cost, tot[0], tb[0])
    # the bound is tight enough to mean something: a relative 1e-12 of the scale
    assert np.all(bnd <= 1e-14 * 100 * MR.scale(P, x0, ks, dt, discs, vel))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 32])
def test_zero_velocity_is_the_static_reference_exactly(n):
    x0, discs, vel, P, ks, dt = scene(n, 300 + n, still=True)
    for backend in (None, "exact"):
        a, b = MR.power(P, ks, dt, discs, vel, backend=backend), OR.power(P, discs, backend=backend)
        assert same_ld(a, b)
    assert same_ld(MR.power(P, ks, dt, discs, None), OR.power(P, discs))
    np.testing.assert_array_equal(MR.scale(P, x0, ks, dt, discs, vel), OR.scale(P, x0, discs))
    ta, tb = MR.sample_penalty(P[None], x0, ks, dt, discs, vel, 3.0), OR.sample_penalty(P[None], x0, discs, 3.0)
    assert same_ld(ta[0], tb[0])
    # ... and so is the spec: at = a, bt = b, ct = c exactly
    s_m, c_m = spec(P, ks, x0, dt, discs, vel, 3.0)
    s_o, c_o = OC.spec(P, x0, discs, 3.0)
    assert s_m.tobytes() == s_o.tobytes() and c_m == c_o


def test_longdouble_and_exact_backends_agree():
    x0, discs, vel, P, ks, dt = scene(4, 5, 127)
    a, b = MR.power(P, ks, dt, discs, vel), MR.power(P, ks, dt, discs, vel, backend="exact")
    assert np.all(np.abs(a - b) <= MR.REF_ULPS * 2.0 ** -64 * MR.scale(P, x0, ks, dt, discs, vel))
    np.testing.assert_array_equal(MR.penalty(P, ks, dt, discs, vel, 0.0), np.zeros(len(P)))


def test_nan_state_and_zero_weight():
    x0, discs, vel, P, ks, dt = scene(3, 9)
    P = np.concatenate([P, [[np.nan, 1.0], [2.0, np.nan], [np.nan, np.nan]]])
    ks = np.concatenate([ks, [3, 9, 14]])
    s, cost = spec(P, ks, x0, dt, discs, vel, 3.0)
    assert np.all(np.isnan(s[-3:])) and math.isfinite(cost)
    pen = MR.penalty(P, ks, dt, discs, vel, 3.0)
    assert np.all(pen[-3:] == 0) and np.all(MR.bound_penalty(P, x0, ks, dt, discs, vel, 3.0)[-3:] == 0)
    tot, tb = MR.sample_penalty(P[None], x0, ks, dt, discs, vel, 3.0)
    assert abs(LD(cost) - tot[0]) <= tb[0]
    _, c0 = spec(P, ks, x0, dt, discs, vel, 0.0)
    assert c0 == 0.0 and MR.sample_penalty(P[None], x0, ks, dt, discs, vel, 0.0)[0][0] == 0


def crossing_sample():
    """one sample of 15 states driving along x at 1.2 m/s, dt = 0.1, and a disc of 0.3 m that crosses its path at (-0.5, 1.1)
    m/s and is centred on state 10 at step 10: states 9 .. 11 penetrate, every one of them at a step past the first block of eight"""
    x0 = np.array([3.0, -2.0])
    dt, ks = 0.1, np.arange(15)
    P = np.stack([x0[0] + 0.12 * ks, x0[1] + 0.01 * ks], axis=1)
    vel = np.array([[-0.5, 1.1], [0.3, -0.2]])
    discs = np.array([[0.0, 0.0, 0.3], [x0[0] + 9.0, x0[1] + 9.0, 0.5]])
    discs[0, :2] = P[10] - vel[0] * (10 * dt)
    return x0, discs, vel, P, ks, dt


@pytest.mark.parametrize("wrong", ["late", "local", "sign", "nodt", "notau2", "cross1", "xonly"])
def test_wrong_versions_are_outside(wrong):
    """tau one step late (k + 1); the index inside the block of eight in place of the global step; the sign of v; dt left out
    of tau; the tau^2 term of c dropped; the cross term without its factor 2; the velocity applied to x only"""
    x0, discs, vel, P, ks, dt = crossing_sample()
    w = 7.5
    tot, tb = MR.sample_penalty(P[None], x0, ks, dt, discs, vel, w)
    ref_s = MR.power(P, ks, dt, discs, vel)
    assert np.count_nonzero(ref_s[9:12] < 0) == 3 and np.all(ref_s[:8] > 0) and tot[0] > 0.1
    s, cost = spec(P, ks, x0, dt, discs, vel, w, wrong)
    assert abs(LD(cost) - tot[0]) > tb[0], (wrong, cost, tot[0], tb[0])
    assert np.any(np.abs(s.astype(LD) - ref_s).astype(np.float64) > MR.bound_s(P, x0, ks, dt, discs, vel))
    # ... and the right one is inside, on the same sample
    s, cost = spec(P, ks, x0, dt, discs, vel, w)
    assert abs(LD(cost) - tot[0]) <= tb[0]
    assert np.all(np.abs(s.astype(LD) - ref_s).astype(np.float64) <= MR.bound_s(P, x0, ks, dt, discs, vel))


# ---- the interface, CPU side ---------------------------------------------------------------------------------------------
def test_moving_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert MOVING <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in MOVING:
        assert hasattr(lib, name), "libccv_mppi_hip.so does not export %s" % name
        assert name in capi.SIGNATURES
        assert capi.SIGNATURES[name][1][2] is C.c_int32
    assert capi.BATCH_KERNEL_MOVING == int(re.search(r"#define CCV_MPPI_BATCH_KERNEL_MOVING (\d+)", text).group(1)) == 256
    assert capi.BATCH_KERNEL_MOVING & (capi.BATCH_KERNEL_ONE_WAVE | capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE |
                                       capi.BATCH_KERNEL_VARIED | capi.BATCH_KERNEL_SHIFT | capi.BATCH_KERNEL_OBST) == 0


def test_moving_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_moving.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, const double*, int32_t);\n'
        'typedef int (*get_fn)(ccv_mppi_batch*, double*, int32_t);\n'
        'int main(void){set_fn a = ccv_mppi_batch_set_obstacle_velocities; get_fn b = ccv_mppi_batch_get_obstacle_velocities;\n'
        'return (a && b && CCV_MPPI_BATCH_KERNEL_MOVING == 256) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_moving.o")], check=True)


def test_a_null_batch_handle_is_refused():
    lib = capi.load()
    vxy = np.zeros((1, 1, 2))
    assert lib.ccv_mppi_batch_set_obstacle_velocities(None, capi.dptr(vxy), 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_set_obstacle_velocities(None, None, 0) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_obstacle_velocities(None, capi.dptr(vxy), 1) == capi.ERR_INVALID_ARG


def test_the_python_class_offers_the_term():
    assert callable(BatchController.set_obstacle_velocities) and callable(BatchController.get_obstacle_velocities)
    import inspect
    assert inspect.signature(BatchController.set_obstacles).parameters["velocities"].default is None


def test_pack_velocities_marshals_and_refuses():
    vel = [np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), [], [(7.0, 8.0)], None]
    vxy, max_n = batch.pack_velocities(vel, 4)
    assert vxy.shape == (4, 3, 2) and vxy.dtype == np.float64 and vxy.flags["C_CONTIGUOUS"] and max_n == 3
    np.testing.assert_array_equal(vxy[0], vel[0])
    np.testing.assert_array_equal(vxy[2, 0], (7.0, 8.0))
    assert not vxy[1].any() and not vxy[2, 1:].any() and not vxy[3].any()
    assert vxy.ravel()[(2 * max_n + 0) * 2:(2 * max_n + 0) * 2 + 2].tolist() == [7.0, 8.0]   # (b, j) at (b * max_n + j) * 2
    batch.pack_velocities(vel, 4, counts=[3, 0, 1, 0])
    with pytest.raises(ValueError):
        batch.pack_velocities(vel, 4, counts=[3, 0, 2, 0])                   # a row count that is not the disc count
    with pytest.raises(ValueError):
        batch.pack_velocities([[]], 2)                                       # one array for two instances
    with pytest.raises(ValueError):
        batch.pack_velocities([[(1.0, 2.0, 3.0)]], 1)                        # not pairs
    with pytest.raises(ValueError):
        batch.pack_velocities([np.zeros((capi.MAX_OBSTACLES + 1, 2))], 1)


# ---- fleet prediction, CPU side -------------------------------------------------------------------------------------------
import fleet_reference as FR  # noqa: E402
import fleet_velocity_reference as FV  # noqa: E402

PRED = {"ccv_mppi_batch_set_fleet_prediction", "ccv_mppi_batch_get_fleet_prediction", "ccv_mppi_batch_read_fleet_velocities"}


@pytest.mark.parametrize("dt,advance", [(0.1, True), (0.1, False), (0.0, True), (0.105, True), (1e-310, True), (5e-324, True)])
def test_fleet_velocity_rule_backends_agree(dt, advance):
    """advance on and off, dt = 0, two values of dt whose reciprocal overflows (the overflowing quotient under a finite
    reciprocal: the next test)"""
    rng = np.random.default_rng(7)
    before = rng.uniform(-50, 50, (40, 2))
    after = before + rng.uniform(-0.2, 0.2, (40, 2))
    after[3] = before[3]                      # a robot that did not move
    a, b = FV.velocity(before, after, dt, advance), FV.velocity_exact(before, after, dt, advance)
    assert a.tobytes() == b.tobytes()
    if not advance or dt == 0.0 or dt < 1e-305:
        assert not a.any()
    else:
        assert np.all(np.isfinite(a)) and a[5].any() and not a[3].any()
        np.testing.assert_allclose(a, (after - before) / dt, rtol=4e-16)


def test_fleet_velocity_zeroes_both_components_together():
    before, after = np.array([[0.0, 0.0]]), np.array([[1e10, 1e-10]])
    assert np.isfinite(1.0 / 1e-300)
    assert not FV.velocity(before, after, 1e-300, True).any()      # vx = 1e10 * 1e300 overflows: vy goes with it
    assert not FV.velocity_exact(before, after, 1e-300, True).any()
    assert FV.velocity(before, np.array([[1.0, 1e-10]]), 1e-300, True).all()


def test_fleet_velocity_lists_carry_the_reference_selection():
    rng = np.random.default_rng(3)
    q = rng.uniform(0, 3, (12, 2))
    radius, n_static = rng.uniform(0.1, 0.3, 12), np.array([0, 30, 32] * 4, dtype=np.int32)
    n_total, rows, taken = FV.lists(q, radius, n_static, 4, 1.5)
    want_n, want_rows = FR.lists(q, radius, n_static, 4, 1.5)
    np.testing.assert_array_equal(n_total, want_n)
    assert all(np.array_equal(a, b) for a, b in zip(rows, want_rows))
    assert [len(t) for t in taken] == (n_total - n_static).tolist() and all(y not in t for y, t in enumerate(taken))
    v = rng.uniform(-1, 1, (12, 2))
    tab = FV.table(FV.velocity_rows([np.zeros((int(n), 2)) for n in n_static], taken, v))
    assert tab.shape == (12, 32, 2) and np.array_equal(tab[0, :len(taken[0])], v[taken[0]]) and not tab[2].any()


def test_prediction_symbols_are_declared_exported_and_in_the_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert PRED <= set(re.findall(r"\b(ccv_mppi_batch_[a-z_0-9]+)\s*\(", src))
    lib = C.CDLL(build.build())
    for name in PRED:
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
        assert not name.startswith("ccv_mppi_batch_resident_") and name not in capi.FLEET_SIGNATURES
    lib = capi.load()
    assert lib.ccv_mppi_batch_set_fleet_prediction(None, 1) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_get_fleet_prediction(None) == capi.ERR_INVALID_ARG
    assert lib.ccv_mppi_batch_read_fleet_velocities(None, capi.dptr(np.zeros((1, 32, 2)))) == capi.ERR_INVALID_ARG
    assert callable(BatchController.resident_set_fleet_prediction) and callable(BatchController.resident_read_fleet_velocities)


def test_prediction_header_compiles_as_c99(tmp_path):
    src = tmp_path / "batch_pred.c"
    src.write_text(
        '#include <stddef.h>\n#include "ccv_mppi.h"\n'
        'typedef int (*set_fn)(ccv_mppi_batch*, int32_t);\ntypedef int (*get_fn)(const ccv_mppi_batch*);\n'
        'typedef int (*read_fn)(ccv_mppi_batch*, double*);\n'
        'int main(void){set_fn a = ccv_mppi_batch_set_fleet_prediction; get_fn b = ccv_mppi_batch_get_fleet_prediction;\n'
        'read_fn c = ccv_mppi_batch_read_fleet_velocities; return (a && b && c) ? 0 : 1;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "batch_pred.o")], check=True)

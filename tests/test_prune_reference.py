"""CPU tests of the specification of the window pruning (tests/prune_reference.py) and of the probe windows
(tests/prune_probe.py) on synthetic fans: the model is sound on every probe and on 2 000 awkward windows, every wrong version
of it is caught (or shown to be sound all the same: prune_reference.SOUND), the pruning is not vacuous, and the fp32 FMA of
the model rounds once.  DESIGN.md section 13.  -s prints the tables."""
import math

import numpy as np
import pytest

import prune_probe as PP
import prune_reference as PR

HS = (17, 20, 50, 63, 64, 65, 68, 127, 128)
KINDS = ("random", "circle", "duplicates", "far", "line_behind", "nan_point", "inf_point", "huge", "nan_position", "inf_position")


def awkward(kind, H, rng, px, py):
    """the windows of tests/test_gpu_parity.py's pruning test about the origin, and two kinds of positions that are not finite"""
    px, py = px.copy(), py.copy()
    if kind == "random":
        w = rng.uniform(-3, 3, H), rng.uniform(-3, 3, H)
    elif kind == "circle":
        a = np.linspace(0, 2 * np.pi, H, endpoint=False)
        w = 1.5 * np.cos(a), 1.5 * np.sin(a)
    elif kind == "duplicates":
        w = np.full(H, 1.0), np.full(H, 0.5)
        w[0][::7] += 0.8
    elif kind == "far":
        w = np.linspace(150.0, 160.0, H), np.linspace(-90.0, -80.0, H)
    elif kind == "line_behind":
        w = -np.linspace(0.0, 4.0, H), np.full(H, 0.2)
    elif kind == "nan_point":
        w = rng.uniform(-2, 2, H), rng.uniform(-2, 2, H)
        w[0][H // 3], w[1][2 * H // 3] = np.nan, np.nan
    elif kind == "inf_point":
        w = np.linspace(0.0, 5.0, H), np.zeros(H)
        w[0][H // 2], w[1][H - 2] = np.inf, -np.inf
    elif kind == "huge":
        w = np.linspace(0.0, 5.0, H) * 1e150, np.linspace(-1.0, 1.0, H) * 1e150
    else:
        w = rng.uniform(-3, 3, H), rng.uniform(-3, 3, H)
        lanes = rng.choice(64, 3, replace=False)
        px[rng.integers(px.shape[0]), lanes[0]] = np.nan if kind == "nan_position" else np.inf
        py[rng.integers(px.shape[0]), lanes[1]] = np.nan if kind == "nan_position" else -np.inf
        px[:, lanes[2]] = np.nan if kind == "nan_position" else np.inf
    return px, py, w[0], w[1]


def judge(px, py, xr, yr, H, wrong=None, full=None):
    a, b, c = PR.window_coeffs(xr, yr)
    jb, je, keep, jr = PR.device_hull(px, py, a, b, c, H, wrong)
    ok, _ = PR.sound((jb, je), px, py, a, b, c, H, full)
    return ok, (jb, je)


def probes_of(P, H, blocks):
    """every probe of prune_probe on the given blocks of the fan P -> a list of (what, px, py, Probe, small: the builder
    promises a hull below H4)"""
    out = []
    for bn in blocks:
        px, py = PP.block_of(P, bn)
        for side in PP.SIDES:
            if PP.extreme(px, py, side) is None:
                continue
            for k in (PP.RUNGS if side == "xhi" else (2, 10, 30)):
                out.append(("b%d" % bn, px, py, PP.ladder(px, py, H, side, k), True))
            if PP.fp32_rounds_inwards(px, py, side):
                try:
                    out.append(("b%d" % bn, px, py, PP.fp32_gap(px, py, H, side), True))
                except AssertionError as e:   # (a gap too narrow to matter, or the live point a dominator for every t)
                    assert "fp32 gap" in str(e), e
        for j, r, twin in PP.edge_cases(H):
            out.append(("b%d" % bn, px, py, PP.edge(px, py, H, j, r, twin), True))
        out.append(("b%d" % bn, px, py, PP.two_live(px, py, H)[0], False))
        out.append(("b%d" % bn, px, py, PP.single_survivor(px, py, H), True))
        out.append(("b%d" % bn, px, py, PP.pose_point(px, py, H), False))
        cx, cy = PP.coincident(px, py)
        out.append(("b%d coincident" % bn, cx, cy, PP.single_survivor(cx, cy, H), True))
        out.append(("b%d coincident" % bn, cx, cy, PP.pose_point(cx, cy, H), False))
        out.append(("b%d coincident" % bn, cx, cy, PP.on_states(cx, cy, H), False))
        out.append(("b%d coincident" % bn, cx, cy, PP.single_survivor(cx, cy, H, twin=True), True))
    return out


def lane_and_nan_probes(P, H, bn):
    """two probes for two wrong versions: the fan's lanes rolled so that p* is lane 63's; a NaN position after p*"""
    px, py = PP.block_of(P, bn)
    star, _ = PP.extreme(px, py, "xhi")
    rolled = np.roll(P, 63 - star % 64, axis=0)
    qx, qy = PP.block_of(rolled, bn)
    assert PP.extreme(qx, qy, "xhi")[0] % 64 == 63
    out = [("b%d lane 63" % bn, qx, qy, PP.ladder(qx, qy, H, "xhi", 10), True)]
    side = next(sd for sd in PP.SIDES if PP.extreme(px, py, sd) is not None and PP.extreme(px, py, sd)[0] < px.size - 64)
    p = PP.ladder(px, py, H, side, 10)
    nx, ny = px.copy(), py.copy()
    nx.ravel()[p.star + 1], ny.ravel()[p.star + 1] = np.nan, np.nan   # (a minimum that lets it in forgets what came before it)
    out.append(("b%d NaN position" % bn, nx, ny, p, True))
    return out


@pytest.fixture(scope="module")
def all_probes():
    out = []
    for H in HS:
        P = PP.synthetic_fan(100 + H, H)
        last = (H - 1) // 8
        blocks = sorted({1, last}) if H in (17, 63, 64, 127) else sorted({0, 1, last // 2, last})
        for what, px, py, p, small in probes_of(P, H, blocks if H in (17, 50, 68, 128) else blocks[-1:]):
            out.append((H, what, px, py, p, small))
        for what, px, py, p, small in lane_and_nan_probes(P, H, max(1, last // 2)):
            out.append((H, what, px, py, p, small))
    return out


def test_fp32_fma_rounds_once():
    """fmaf32 against exact rationals on 10 000 triples, some of them built so that the fp64 detour rounds differently: a b is
    the midpoint of two fp32 neighbours and c a sliver beside it"""
    rng = np.random.default_rng(7)
    n = 10000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    m = 400
    e1, e2 = rng.integers(-8, 9, m), rng.integers(-8, 9, m)
    a[:m] = np.float32(1 + 2.0 ** -12) * np.float32(2.0) ** e1          # a b = (1 + 2^-11 + 2^-24) 2^(e1 + e2): a midpoint
    b[:m] = np.float32(1 + 2.0 ** -12) * np.float32(2.0) ** e2
    c[:m] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * np.float32(2.0) ** (e1 + e2 - 60 - np.arange(m) % 20)
    c[m:2 * m] = -a[m:2 * m] * b[m:2 * m]                               # (cancellation)
    got = PR.fmaf32(a, b, c)
    differ = 0
    for i in range(n):
        want = PR.fmaf32_rational(a[i], b[i], c[i])
        assert got[i] == want, (i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want))
        differ += int(PR.fmaf32_detour(a[i], b[i], c[i]) != want)
    print("[prune] fmaf32: %d triples equal the rationals; the fp64 detour differs on %d" % (n, differ))
    assert differ >= 1


def test_model_is_sound_on_every_probe(all_probes):
    bad = []
    for H, what, px, py, p, small in all_probes:
        ok, hull = judge(px, py, p.xr, p.yr, H)
        if not ok:
            bad.append((H, what, p.what, hull))
    print("[prune] %d probes, the model sound on all but %d" % (len(all_probes), len(bad)))
    assert not bad, bad[:5]


def test_model_is_sound_on_awkward_windows():
    rng = np.random.default_rng(11)
    n, counts = 0, {}
    while n < 2000:
        H = HS[n % len(HS)]
        kind = KINDS[(n // len(HS)) % len(KINDS)]
        P = PP.synthetic_fan(int(rng.integers(1 << 30)), H, noise=float(rng.uniform(0.0, 1.5)))
        bn = int(rng.integers((H + 7) // 8))
        px, py = PP.block_of(P, bn)
        nv = int(rng.integers(1, px.shape[0] + 1))
        px, py, xr, yr = awkward(kind, H, rng, px[:nv], py[:nv])
        ok, hull = judge(px, py, xr, yr, H)
        assert ok, (n, H, kind, bn, nv, hull)
        counts[kind] = counts.get(kind, 0) + (hull != (0, PR.h4_of(H)))
        n += 1
    print("[prune] 2000 awkward windows, the model sound on all; a hull below H4 per kind: %s" % counts)


def test_every_wrong_version_is_caught(all_probes):
    """every entry of WRONG is unsound on a probe, or -- the two that only choose another dominator, which any window point
    may be -- keeps more than the specification does on a probe whose hull the builder promises small; prune_reference.SOUND
    names those, with the reason, and the one that nothing can catch"""
    unsound, wasteful = {w: [] for w in PR.WRONG}, {w: [] for w in PR.WRONG}
    for H, what, px, py, p, small in all_probes:
        a, b, c = PR.window_coeffs(p.xr, p.yr)
        full = PR.loop_minimum(px, py, a, b, c, H)
        spec = PR.device_hull(px, py, a, b, c, H)[:2]
        for w in PR.WRONG:
            hull = PR.device_hull(px, py, a, b, c, H, w)[:2]
            if hull == spec:
                continue
            name = "H%d %s %s" % (H, what, p.what)
            if not PR.sound(hull, px, py, a, b, c, H, full)[0]:
                unsound[w].append(name)
            elif small and hull[0] <= spec[0] and hull[1] >= spec[1]:
                wasteful[w].append(name)
    for w in PR.WRONG:
        print("[prune] wrong %-16s unsound on %4d probes, wasteful on %4d; first: %s"
              % (w, len(unsound[w]), len(wasteful[w]), (unsound[w] + wasteful[w] + ["-"])[0]))
    for w in PR.WRONG:
        if w not in PR.SOUND:
            assert unsound[w], "nothing catches the wrong version %s" % w
        else:
            assert not unsound[w], "%s is listed as sound, and a probe shows it unsound: %s" % (w, unsound[w][:3])
            assert bool(wasteful[w]) == PR.SOUND[w][0], (w, len(wasteful[w]))


def test_pruning_is_not_vacuous(all_probes):
    n_small = 0
    for H, what, px, py, p, small in all_probes:
        a, b, c = PR.window_coeffs(p.xr, p.yr)
        jb, je, keep, jr = PR.device_hull(px, py, a, b, c, H)
        if small:
            assert je - jb < PR.h4_of(H), (H, what, p.what, jb, je)
            n_small += 1
        if "coincident" in what or "lane" in what or "NaN" in what or p.what.startswith(("single", "pose")):   # (no pair of survivors promised)
            continue
        xp, yp, order = PP.permuted(p.xr, p.yr, [(px, py)], H)
        a, b, c = PR.window_coeffs(xp, yp)
        jb, je, _, _ = PR.device_hull(px, py, a, b, c, H)
        assert (jb, je) == (0, PR.h4_of(H)), (H, what, p.what, jb, je)
    assert n_small > 100, n_small
    # a path-like window at H = 50: the share of (state, point) pairs the loop still visits, with the switch
    H = 50
    P = PP.synthetic_fan(5, H, noise=0.5)
    k = np.arange(H)
    xr, yr = 0.06 * k * math.cos(0.3), 0.06 * k * math.sin(0.3) + 0.05 * np.sin(0.2 * k)
    a, b, c = PR.window_coeffs(xr, yr)
    blocks = PP.blocks_of(P)
    trace = PR.switch_trace(blocks, a, b, c, H)
    kept = sum(len(px) * (je - jb) for (px, _), (jb, je, _) in zip(blocks, trace))
    share = kept / float(sum(len(px) for px, _ in blocks) * PR.h4_of(H))
    print("[prune] path window, H = 50: %.1f %% of the pairs remain; hulls %s" % (100.0 * share, [(jb, je) for jb, je, _ in trace]))
    assert share < 0.60, share

"""The prologue of a resident tick -- get_CurrentIndex() + calc_RefPath() (dd:126-140, 156-181) -- restated in plain numpy
float64, the cases the prologue tests run (tests/test_prologue_reference.py on the CPU, tests/test_gpu_prologue_sweep.py on
the device), and deliberately wrong versions of the restatement (MUTATIONS) that the case list has to tell apart from it.

No product code is used here.  The device kernels split the scan of the path over NT threads (thread t takes the indices
i with i % NT == t, four per outer round) and reduce (distance, index) pairs; the restatement is the serial scan they must
reproduce, and the mutations that model a wrong reduction take NT as the kernels have it (256 and 1024).
"""
import numpy as np

GATE = 100.0
NTS = (256, 1024)        # the two widths advance_body is compiled with
K_LOADS = 4              # path poses per thread and outer round of the scan
DEFAULT = dict(v_ref=0.8, dt=0.1, resolution=0.1)


def distances(px, py, x, y):
    ex, ey = x - np.asarray(px, dtype=np.float64), y - np.asarray(py, dtype=np.float64)
    return np.sqrt(ex * ex + ey * ey)


def nearest_index(px, py, x, y):
    """The serial scan: strict '<' against a running minimum that starts at the gate; 0 when nothing qualifies."""
    best, index = GATE, 0
    for i, d in enumerate(distances(px, py, x, y).tolist()):
        if d < best:
            best, index = d, i
    return index


def ref_window(px, py, x, y, v_ref, dt, resolution, H):
    """(index, x_ref[H], y_ref[H], (s0, s1)): window point i is path pose min(int(start + i * (v_ref * dt / resolution)),
    n_path - 1); s0, s1 are the poses of window points 0 and 1, the two yaw_ref0 = atan2(y[s1] - y[s0], x[s1] - x[s0]) reads."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    start = nearest_index(px, py, x, y)
    stride = float(v_ref) * float(dt) / float(resolution)
    src = [min(int(start + i * stride), len(px) - 1) for i in range(H)]
    return start, px[src].copy(), py[src].copy(), (src[0], src[1])


def batch_ref(path_x, path_y, lengths, poses, v_ref, dt, resolution, H):
    """B instances whose paths lie back to back in path_x / path_y: ref_window of each on its own slice."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [ref_window(path_x[off[b]:off[b + 1]], path_y[off[b]:off[b + 1]], poses[b][0], poses[b][1], v_ref[b], dt,
                       resolution[b], H) for b in range(len(lengths))]


# ---- wrong versions --------------------------------------------------------------------------------------------------------
MUTATIONS = (
    "tie_keeps_last", "gate_inclusive", "squared_distances", "lower_thread_wins_nt256", "lower_thread_wins_nt1024",
    "first_4nt_only_nt256", "first_4nt_only_nt1024", "stride_other_association", "start_plus_int", "round_not_truncate",
    "window_wraps", "clamp_n_minus_2", "instance0_v_ref", "instance0_resolution", "slice_one_early", "slice_one_late")
BATCH_MUTATIONS = ("instance0_v_ref", "instance0_resolution", "slice_one_early", "slice_one_late")


def _mutated_index(name, px, py, x, y):
    d = distances(px, py, x, y)
    if name == "squared_distances":
        ex, ey = x - px, y - py
        d = ex * ex + ey * ey
        gate = GATE * GATE
    else:
        gate = GATE
    if name.startswith("first_4nt_only"):
        nt = int(name.rsplit("nt", 1)[1])
        d = d[:K_LOADS * nt]
    if name.startswith("lower_thread_wins"):
        nt = int(name.rsplit("nt", 1)[1])
        best = [(gate, -1)] * nt                       # per thread: the first of its equal distances (ascending i)
        for i, v in enumerate(d.tolist()):
            if v < best[i % nt][0]:
                best[i % nt] = (v, i)
        m = min(b[0] for b in best)
        index = next(b[1] for b in best if b[0] == m)   # the lowest thread id that holds the minimum
        return max(index, 0)
    best, index, found = gate, 0, False
    for i, v in enumerate(d.tolist()):
        if name == "tie_keeps_last":
            take = v < best or (found and v == best)
        elif name == "gate_inclusive":
            take = v < best or (not found and v == best)
        else:
            take = v < best
        if take:
            best, index, found = v, i, True
    return index


def mutated(name, px, py, x, y, v_ref, dt, resolution, H):
    """ref_window with one thing wrong; the batch mutations are the identity here (mutated_batch)."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    n = len(px)
    start = _mutated_index(name, px, py, x, y)
    v_ref, dt, resolution = float(v_ref), float(dt), float(resolution)
    stride = v_ref * (dt / resolution) if name == "stride_other_association" else v_ref * dt / resolution
    src = []
    for i in range(H):
        if name == "start_plus_int":
            idx = start + int(i * stride)
        elif name == "round_not_truncate":
            idx = int(np.floor(start + i * stride + 0.5))
        else:
            idx = int(start + i * stride)
        if name == "window_wraps":
            idx = idx % n
        elif name == "clamp_n_minus_2":
            idx = min(idx, max(n - 2, 0))
        src.append(min(idx, n - 1))
    return start, px[src].copy(), py[src].copy(), (src[0], src[1])


def mutated_batch(name, path_x, path_y, lengths, poses, v_ref, dt, resolution, H):
    """batch_ref with one thing wrong (a name outside BATCH_MUTATIONS: every instance through mutated())."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    total = int(off[-1])
    out = []
    for b in range(len(lengths)):
        lo, hi = int(off[b]), int(off[b + 1])
        v, r = v_ref[b], resolution[b]
        if name == "instance0_v_ref":
            v = v_ref[0]
        elif name == "instance0_resolution":
            r = resolution[0]
        elif name == "slice_one_early":
            lo, hi = max(lo - 1, 0), max(lo - 1, 0) + (hi - lo)
        elif name == "slice_one_late":
            hi = min(hi + 1, total)
        fn = ref_window if name in BATCH_MUTATIONS else (lambda *a: mutated(name, *a))
        out.append(fn(path_x[lo:hi], path_y[lo:hi], poses[b][0], poses[b][1], v, dt, r, H))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def base_path(m, x0=0.0):
    """m distinct poses 0.1 m apart along x with a small ripple in y: pose j + (0.01, 0.02) is nearest to j alone."""
    k = np.arange(m, dtype=np.float64)
    return x0 + 0.1 * k, 0.003 * (np.arange(m) % 7).astype(np.float64)


def near(px, py, j):
    return float(px[j]) + 0.01, float(py[j]) + 0.02


def make_case(name, group, px, py, pose, H=9, expect=None, moving=False, **kw):
    c = dict(DEFAULT)
    c.update(kw)
    c.update(name=name, group=group, px=np.ascontiguousarray(px, dtype=np.float64), py=np.ascontiguousarray(py, dtype=np.float64),
             x=float(pose[0]), y=float(pose[1]), H=H, expect=expect, moving=moving)
    return c


LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 4095, 4096, 4097)
TIE_LENGTHS = (256, 1024, 4096, 252, 192, 1020, 960, 65)
STRIDES = ((0.7, 0.1, 0.1), (0.3, 0.3, 0.1), (1.0, 0.1, 0.1), (1.2, 0.1, 0.1), (0.8, 0.0, 0.1))
BATCH_LENGTHS = (1, 2, 255, 257, 1025)
BATCH_RESOLUTION = (0.1, 0.05, 0.1, 0.03, 0.1)
BATCH_V_REF = (0.7, 0.3, 1.0, 1.2, 0.7)


def length_targets(n):
    top = ((n - 1) // 256) * 256            # the largest multiple of 256 below n_path
    want = {0, n - 1, top - 1, top, top + 1}
    return sorted(j for j in want if 0 <= j < n)


def gate_offsets():
    """{(kind, axis): (ox, oy)}: offsets of a lone candidate from the pose whose np.sqrt distance is exactly 100.0 (`on`), the
    double below it (`inside`) and the double above it (`outside`), from the (60, 80) and the (100, 0) construction.  Found by
    stepping one coordinate a double at a time, not assumed."""
    out = {}
    for axis, (ox, oy) in (("60_80", (60.0, 80.0)), ("100_0", (100.0, 0.0))):
        out[("on", axis)] = (ox, oy)
        for kind, toward, want in (("inside", 0.0, np.nextafter(GATE, 0.0)), ("outside", np.inf, np.nextafter(GATE, np.inf))):
            a, b = ox, oy
            for _ in range(64):
                if axis == "60_80":
                    b = float(np.nextafter(b, toward))
                else:
                    a = float(np.nextafter(a, toward))
                if float(np.sqrt(a * a + b * b)) == want:
                    break
            out[(kind, axis)] = (a, b)
    return out


def sqrt_pair(one_ulp):
    """Offsets (a, b) of two path poses from the pose (0, 0).  one_ulp False: different squares a.a, b.b with the same np.sqrt
    (a has the larger square); True: np.sqrt differs by exactly one ulp (a is the farther one)."""
    for k in range(1, 4000):
        bx, by = 3.0 + 0.001 * k, 4.0
        ax = float(np.nextafter(bx, np.inf))
        sa, sb = ax * ax + by * by, bx * bx + by * by
        da, db = float(np.sqrt(sa)), float(np.sqrt(sb))
        if not one_ulp and sa > sb and da == db:
            return (ax, by), (bx, by)
        if one_ulp and da == float(np.nextafter(db, np.inf)):
            return (ax, by), (bx, by)
    raise AssertionError("no pair found")


def far_points(n):
    """n poses far outside the gate of the pose (0, 0) the gate / sqrt cases use"""
    return 500.0 + np.arange(n, dtype=np.float64), np.full(n, 400.0)


def cases():
    out = []
    # length residues: every length with the nearest pose at its ends and around the last multiple of 256
    for n in LENGTHS:
        px, py = base_path(n)
        for j in length_targets(n):
            out.append(make_case("len%d_at%d" % (n, j), "length", px, py, near(px, py, j), H=9 if (n + j) % 2 else 30, expect=j))
    # ties by construction: exact copies of coordinates
    for m in TIE_LENGTHS:
        P = base_path(m)
        px, py = np.concatenate([P[0], P[0]]), np.concatenate([P[1], P[1]])
        for j in sorted({0, 5, min(70, m - 2), m - 1}):
            out.append(make_case("tie_pp%d_at%d" % (m, j), "tie", px, py, near(px, py, j), H=9 if j % 2 else 30, expect=j, moving=j == 5))
    P = base_path(300)
    for j in (0, 7, 299):
        out.append(make_case("tie_repeat_at%d" % j, "tie", np.repeat(P[0], 2), np.repeat(P[1], 2), near(P[0], P[1], j), expect=2 * j,
                         moving=j == 7))
    out.append(make_case("tie_threads_63_64", "tie", np.concatenate([P[0][:1], np.repeat(P[0][1:], 2)]),
                     np.concatenate([P[1][:1], np.repeat(P[1][1:], 2)]), near(P[0], P[1], 32), expect=63))
    P = base_path(700)
    for j in (3, 350, 699):
        out.append(make_case("tie_reversed_at%d" % j, "tie", np.concatenate([P[0], P[0][::-1]]), np.concatenate([P[1], P[1][::-1]]),
                         near(P[0], P[1], j), H=30, expect=j, moving=j == 3))
    for m in (300, 4096):
        P = base_path(m)
        for j in (4, m - 1):
            out.append(make_case("tie_ppp%d_at%d" % (m, j), "tie", np.tile(P[0], 3), np.tile(P[1], 3), near(P[0], P[1], j), expect=j,
                             moving=(m, j) == (300, 4)))
    # gate: a lone candidate at index 5; every other pose is outside the gate
    for (kind, axis), (ox, oy) in sorted(gate_offsets().items()):
        px, py = far_points(12)
        px[5], py[5] = ox, oy
        out.append(make_case("gate_%s_%s" % (kind, axis), "gate", px, py, (0.0, 0.0), expect=5 if kind == "inside" else 0))
    # distances that differ only before the sqrt (the larger square at the lower index), and by one ulp after it (the nearer
    # pose at the higher index)
    for one_ulp in (False, True):
        a, b = sqrt_pair(one_ulp)
        for lo, hi, n in ((2, 7, 12), (3, 700, 900)):
            px, py = far_points(n)
            px[lo], py[lo], px[hi], py[hi] = a[0], a[1], b[0], b[1]
            out.append(make_case("%s_%d_%d" % ("one_ulp" if one_ulp else "same_sqrt", lo, hi), "one_ulp" if one_ulp else "same_sqrt", px, py,
                             (0.0, 0.0), expect=hi if one_ulp else lo))
    # stride: the truncated index by association and by the size of start
    px, py = base_path(1200)
    for v_ref, dt, res in STRIDES:
        for start in (0, 3, 1000, 1003):
            for H in (9, 30):
                out.append(make_case("stride_v%g_dt%g_at%d_H%d" % (v_ref, dt, start, H), "stride", px, py, near(px, py, start), H=H, expect=start,
                                 v_ref=v_ref, dt=dt, resolution=res))
    # path end: the final pose repeats
    px, py = base_path(40)
    for back in (1, 2, 3):
        for H in (9, 30):
            out.append(make_case("end_minus%d_H%d" % (back, H), "end", px, py, near(px, py, 40 - back), H=H, expect=40 - back, moving=True))
    px, py = base_path(5)
    for H in (9, 30):
        out.append(make_case("short5_H%d" % H, "end", px, py, near(px, py, 1), H=H, expect=1, moving=True))
        out.append(make_case("single_pose_H%d" % H, "end", px[:1] + 2.0, py[:1], (2.3, 0.1), H=H, expect=0))
    return out


def batch_layout():
    """B = 5 paths back to back.  Instances 1 to 3 stand where the last pose of the previous path and the first pose of the next
    one are both nearer than any pose of their own path, whose nearest pose (at exactly 1.0 m) is the expected index."""
    B = len(BATCH_LENGTHS)
    q = [(60.0 * b, 7.0) for b in range(B)]
    paths, expect = [], []
    for b, n in enumerate(BATCH_LENGTHS):
        mid = n // 2
        px = q[b][0] + 0.1 * (np.arange(n, dtype=np.float64) - mid)
        py = np.full(n, q[b][1] + 1.0)
        want = mid
        if 1 <= b - 1 <= 3:                    # this path's first pose is a trap for the previous instance
            px[0], py[0] = q[b - 1][0] + 0.05, q[b - 1][1]
        if 1 <= b + 1 <= 3:                    # this path's last pose is a trap for the next instance
            px[-1], py[-1] = q[b + 1][0] - 0.05, q[b + 1][1]
        if n == 2:                             # (instance 1: its first pose is its own nearest, its last the trap)
            want = 0
            px[0], py[0] = q[b][0], q[b][1] + 1.0
        if n == 1:
            want = 0
        paths.append((px, py))
        expect.append(want)
    return dict(paths=paths, poses=q, lengths=BATCH_LENGTHS, resolution=BATCH_RESOLUTION, v_ref=BATCH_V_REF, dt=0.1, expect=expect)


def filler(slot, H, v_ref=DEFAULT["v_ref"], dt=DEFAULT["dt"]):
    """An ordinary instance that fills a batch up: three poses of its own far from every case, the robot next to the middle one"""
    px = -500.0 - 10.0 * slot + 0.1 * np.arange(3, dtype=np.float64)
    py = np.full(3, -300.0)
    return make_case("filler%d" % slot, "filler", px, py, near(px, py, 1), H=H, expect=1, v_ref=v_ref, dt=dt)

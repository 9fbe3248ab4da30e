"""GPU tests (-m gpu): path length, ties, gate and stride through every resident prologue kernel.

The prologue of a resident tick (advance_body, csrc/mppi_update_device.h: plant step, get_CurrentIndex(), calc_RefPath(), window
coefficients) is compiled into thirteen kernels.  The checker is tests/prologue_reference.py -- a serial float64 restatement in
numpy that tests/test_prologue_reference.py holds against the host prologue and the oracle -- and everything it specifies is
compared bit for bit: the index, x_ref, y_ref, and yaw_ref0 where its two poses coincide (exactly 0.0).  Elsewhere yaw_ref0 is the
device atan2 against np.arctan2 to the 4 ulp tests/test_gpu_resident.py grants it.

Which prologue kernel runs cannot be read from a handle.  The rule these tests rely on is `fin_pending` in resident_step
(csrc/capi_resident.hip) and ccv_mppi_batch_resident_step_enqueue (csrc/capi_batch.hip): a resident step leaves its update
pending, and the next resident step launches that update together with its own prologue (k_finalize_advance*, 256 threads)
unless something flushed it in between -- a read, get_nominal, set_nominal, set_params, a trace read of a batch.  The first
step after a flush launches the prologue kernel of its own (k_advance*: 1024 threads on a single handle, 256 on a batch).  So

  still, first tick   set path(s), warm start and pose(s); one step with advance=False; read           -> k_advance*
  still, fused        the same with two steps back to back, nothing between them; read and trace       -> k_finalize_advance*
  moving, fused       three advance=True steps back to back (duplicate-point paths, path ends); read   -> both, and the plant

and the handle states select the kernel of each column:

  single                               k_advance                    k_finalize_advance
  batch                                k_advance_batch              k_finalize_advance_batch
  batch + set_params                   k_advance_batch_varied       k_finalize_advance_batch_varied
  batch + set_min_shift                k_advance_batch_varied       k_finalize_advance_batch_shift
  batch + fleet                        k_advance_batch_fleet        k_finalize_advance_batch_fleet
  batch + fleet + shift                k_advance_batch_fleet        k_finalize_advance_batch_shift_fleet
  batch + fleet + prediction           k_advance_batch_fleet_pred   k_finalize_advance_batch_fleet_pred
  batch + fleet + prediction + shift   k_advance_batch_fleet_pred   k_finalize_advance_batch_shift_fleet_pred

Every batch state but the first reads v_ref from the parameter table, so all of them get a table with per-instance v_ref
(set_params) on top of what the row names: the kernels are the row's, and a prologue that took the shared v_ref would show.
The fleet states run with weight 0, range 0 and distinct poses: the fleet step runs and adds no disc (asserted).

Batches are B = 5: cases that share dt and H (and v_ref, in the one state without a table) side by side, each on its own path
in the one path array, filled up with small ordinary instances.  K = 64, diff drive; one full-body case per protocol and state.
"""
import numpy as np
import pytest

import ccv_mppi_path_tracker_amd as amd
from ccv_mppi_path_tracker_amd import BatchController, capi, configs
from ccv_mppi_path_tracker_amd.controller import MPPIController
import prologue_reference as PR
import resident_loops as RL

pytestmark = pytest.mark.gpu

K = 64
B = 5
STATES = {
    "single": dict(batch=False),
    "batch": dict(batch=True),
    "batch_params": dict(batch=True, table=True),
    "batch_shift": dict(batch=True, table=True, shift=True),
    "fleet": dict(batch=True, table=True, fleet=True),
    "fleet_shift": dict(batch=True, table=True, fleet=True, shift=True),
    "fleet_pred": dict(batch=True, table=True, fleet=True, pred=True),
    "fleet_pred_shift": dict(batch=True, table=True, fleet=True, pred=True, shift=True),
}
PROTOCOLS = {"still_first": (1, False), "still_fused": (2, False), "moving_fused": (3, True)}   # (steps, advance)
MOVING_V_REF = (0.8, 0.7, 1.0, 1.2, 0.3)        # by slot, where the state has a parameter table
FULL_BODY_CASE = "tie_pp252_at5"                # (moving: the robot drives over doubled poses)
FAR_DISC = np.array([[1.0e4, 1.0e4, 0.5]])

CASES = PR.cases()
LAYOUT = PR.batch_layout()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def params(model, H, v_ref):
    make = {"diff_drive": configs.diff_drive_defaults, "full_body": configs.full_body_defaults}[model]
    return make(K, H).with_(v_ref=v_ref)


def with_v_ref(c, v_ref):
    d = dict(c)
    d["v_ref"] = v_ref
    return d


def chunks(cases, split_v_ref):
    """Lists of B cases that share dt and H (and v_ref), no two with the same pose; short lists filled up."""
    groups = {}
    for c in cases:
        key = (c["dt"], c["H"]) + ((c["v_ref"],) if split_v_ref else ())
        for ch in groups.setdefault(key, []):
            if len(ch) < B and all((c["x"], c["y"]) != (o["x"], o["y"]) for o in ch):
                ch.append(c)
                break
        else:
            groups[key].append([c])
    out = []
    for key, lst in groups.items():
        for ch in lst:
            v = key[2] if split_v_ref else PR.DEFAULT["v_ref"]
            out.append(ch + [PR.filler(s, key[1], v, key[0]) for s in range(len(ch), B)])
    return out


def pose_of(c, nstate):
    s = np.zeros(nstate)
    s[0], s[1] = c["x"], c["y"]
    return s


class Rig:
    """The handles of one state and model, one per H (and v_ref where the handle fixes it), and one way to run a chunk."""

    def __init__(self, state, model="diff_drive"):
        self.cfg, self.model, self.handles = STATES[state], model, {}

    def close(self):
        for h in self.handles.values():
            h.close()

    def handle(self, H, v_ref):
        key = (H, v_ref)
        if key not in self.handles:
            p = params(self.model, H, PR.DEFAULT["v_ref"] if v_ref is None else v_ref)   # (None: the table overrides it)
            if self.cfg["batch"]:
                self.handles[key] = BatchController(p, B, num_samples=K, min_shift=self.cfg.get("shift", False))
            else:
                self.handles[key] = MPPIController(p, num_samples=K)
        return self.handles[key]

    def run(self, chunk, steps, advance):
        """-> per case (state, index, x_ref, y_ref, yaw_ref0, trace rows, u*) after `steps` steps back to back"""
        H, dt = chunk[0]["H"], chunk[0]["dt"]
        if not self.cfg["batch"]:
            (c,) = chunk
            g = self.handle(H, c["v_ref"])
            g.set_nominal(np.zeros((H - 1, g.params.udim)))
            g.resident_set_path(c["px"], c["py"], c["resolution"])
            g.resident_set_pose(pose_of(c, g.params.nstate))
            for it in range(steps):   # (nothing between the steps: the second and third prologue ride on the update launch)
                g.resident_step_enqueue(dt, 11, it, advance=advance)
            st, idx, xr, yr, yaw0, n = g.resident_read()
            assert n == steps
            return [(st, idx, xr, yr, yaw0, g.resident_read_trace(), g.get_nominal())]
        table = self.cfg.get("table", False)
        bat = self.handle(H, None if table else chunk[0]["v_ref"])
        if table:
            bat.set_params([params(self.model, H, c["v_ref"]) for c in chunk])
        bat.set_nominal(np.zeros((B, H - 1, bat.udim)))
        bat.resident_set_paths([(c["px"], c["py"]) for c in chunk], [c["resolution"] for c in chunk])
        bat.resident_set_poses(np.array([pose_of(c, bat.nstate) for c in chunk]), 11 + np.arange(B, dtype=np.uint64))
        if self.cfg.get("fleet") and bat.resident_get_fleet()[2] == 0:
            bat.resident_set_fleet(0.1, 0.0, 1, 0.0)
            if self.cfg.get("pred"):
                bat.resident_set_fleet_prediction(True)
        for it in range(steps):
            bat.resident_step_enqueue(dt, it, advance=advance)
        st, idx, xr, yr, yaw0, n = bat.resident_read()
        assert n == steps
        if self.cfg.get("fleet"):
            ns, nt, _ = bat.resident_read_fleet()
            assert not ns.any() and not nt.any(), "the fleet step added a disc"
        u = bat.get_nominal()
        return [(st[b], int(idx[b]), xr[b], yr[b], yaw0[b], bat.resident_read_trace(b), u[b]) for b in range(B)]


def check_window(c, got, x, y, bad):
    """index, x_ref, y_ref bit for bit against the restatement at pose (x, y); yaw_ref0 exactly 0.0 or within 4 ulp"""
    st, idx, xr, yr, yaw0 = got[:5]
    widx, wxr, wyr, (s0, s1) = PR.ref_window(c["px"], c["py"], x, y, c["v_ref"], c["dt"], c["resolution"], c["H"])
    if idx != widx:
        bad.append("%s: index %d, expected %d" % (c["name"], idx, widx))
    if not (np.array_equal(xr, wxr) and np.array_equal(yr, wyr)):
        bad.append("%s: window differs at %s" % (c["name"], np.flatnonzero((xr != wxr) | (yr != wyr)).tolist()))
    if s0 == s1:
        if not (yaw0 == 0.0 and not np.signbit(yaw0)):
            bad.append("%s: yaw_ref0 %r where its two poses coincide" % (c["name"], yaw0))
    else:
        want = np.arctan2(c["py"][s1] - c["py"][s0], c["px"][s1] - c["px"][s0])
        if not abs(yaw0 - want) <= 4 * np.spacing(abs(want)):
            bad.append("%s: yaw_ref0 %r, expected %r" % (c["name"], yaw0, want))


def check_still(c, got, steps, bad):
    st, idx = got[0], got[1]
    if not np.array_equal(st[:2], [c["x"], c["y"]]) or np.any(st[2:] != 0.0):
        bad.append("%s: the pose read back is %s" % (c["name"], st))
    if c["expect"] is not None and idx != c["expect"]:
        bad.append("%s: index %d, the case expects %d" % (c["name"], idx, c["expect"]))
    check_window(c, got, c["x"], c["y"], bad)
    tr = got[5]
    if tr.shape != (steps, 6) or np.any(tr[:, 5] != idx) or np.any(tr[:, 0] != c["x"]) or np.any(tr[:, 1] != c["y"]):
        bad.append("%s: trace rows %s" % (c["name"], tr[:, [0, 1, 5]].tolist()))


def twin_loop(cfg, model, chunk, ticks):
    """The same closed loop with the prologue on the host (ccv_mppi_plant_step, ccv_mppi_calc_ref_path, then the batch's iterate
    in the same weight mode, with the same table and -- for the fleet states -- the kernels of the disc term: one disc far away at
    weight 0, standing still under prediction) -> per tick (poses [B], u* [B])"""
    H, dt = chunk[0]["H"], chunk[0]["dt"]
    table = cfg.get("table", False)
    p = params(model, H, PR.DEFAULT["v_ref"] if table else chunk[0]["v_ref"])
    bat = BatchController(p, B, num_samples=K, min_shift=cfg.get("shift", False))
    if table:
        bat.set_params([params(model, H, c["v_ref"]) for c in chunk])
    if cfg.get("fleet"):
        bat.set_obstacles([FAR_DISC] * B, 0.0, velocities=[np.zeros((1, 2))] * B if cfg.get("pred") else None)
    s = np.array([pose_of(c, p.nstate) for c in chunk])
    u = np.zeros((B, H - 1, p.udim))
    out = []
    for it in range(ticks):
        s = np.array([amd.plant_step(p.model, s[b], u[b][0], dt) for b in range(B)])
        xr, yr, yaw0 = np.zeros((B, H)), np.zeros((B, H)), np.zeros(B)
        for b, c in enumerate(chunk):
            _, xr[b], yr[b], yaw = amd.calc_ref_path(c["px"], c["py"], s[b, 0], s[b, 1], c["v_ref"], dt, c["resolution"], H)
            yaw0[b] = yaw[0]
        u = bat.iterate(s, dt, xr, yr, yaw0, 11 + np.arange(B, dtype=np.uint64), it, want_stats=False)
        out.append((s.copy(), u.copy()))
    bat.close()
    return out


def check_moving(cfg, model, chunk, got, ticks, bad):
    if cfg["batch"]:
        want = twin_loop(cfg, model, chunk, ticks)
        poses = [np.array([w[0][b] for w in want]) for b in range(B)]
        us = [want[-1][1][b] for b in range(B)]
    else:
        (c,) = chunk
        p = params(model, c["H"], c["v_ref"])
        wp, _, wu = RL.host_loop(p.with_(resolution=c["resolution"]), c["px"], c["py"], pose_of(c, p.nstate), ticks, 11, K)
        poses, us = [np.array(wp)], [wu[-1]]
    for b, c in enumerate(chunk):
        st, idx, xr, yr, yaw0, tr, u = got[b]
        n = len(st)
        if tr.shape != (ticks, 6):
            bad.append("%s: %d trace rows" % (c["name"], len(tr)))
            continue
        for row in tr:   # every tick's index is the restatement's at that tick's pose
            want_idx = PR.nearest_index(c["px"], c["py"], row[0], row[1])
            if row[5] != want_idx:
                bad.append("%s: trace index %d at (%r, %r), expected %d" % (c["name"], row[5], row[0], row[1], want_idx))
        if not np.array_equal(tr[-1, :n], st):
            bad.append("%s: the last trace row is not the pose read back" % c["name"])
        check_window(c, got[b], st[0], st[1], bad)
        if model == "diff_drive":   # specified arithmetic end to end: the window coefficients reached the rollout
            if not np.array_equal(tr[:, :n], poses[b]):
                bad.append("%s: poses differ from the host-prologue loop" % c["name"])
            if not np.array_equal(u, us[b]):
                bad.append("%s: u* differs from the host-prologue loop" % c["name"])
        else:             # (fb:408 reads yaw_ref0: the tolerances of test_resident_loop_full_body_within_tolerance)
            if not (np.allclose(tr[:, :n], poses[b], rtol=0, atol=1e-9) and np.allclose(u, us[b], rtol=1e-7, atol=1e-9)):
                bad.append("%s: poses or u* away from the host-prologue loop" % c["name"])
        if np.array_equal(tr[-1, :2], tr[0, :2]):
            bad.append("%s: the robot did not move" % c["name"])


def run_protocol(state, protocol, model, cases):
    steps, advance = PROTOCOLS[protocol]
    cfg = STATES[state]
    if protocol == "moving_fused":
        cases = [c for c in cases if c["moving"]]
    if not cfg["batch"]:
        work = [[c] for c in cases]
    else:
        work = chunks(cases, split_v_ref=not cfg.get("table", False))
        if protocol == "moving_fused" and cfg.get("table"):   # (per-instance v_ref while the robots drive)
            work = [[with_v_ref(c, MOVING_V_REF[s]) for s, c in enumerate(ch)] for ch in work]
    rig, bad = Rig(state, model), []
    try:
        for chunk in work:
            got = rig.run(chunk, steps, advance)
            if advance:
                check_moving(cfg, model, chunk, got, steps, bad)
            else:
                for c, g in zip(chunk, got):
                    check_still(c, g, steps, bad)
    finally:
        rig.close()
    return bad, sum(len(ch) for ch in work)


@pytest.mark.parametrize("protocol", list(PROTOCOLS))
@pytest.mark.parametrize("state", list(STATES))
def test_prologue_sweep(state, protocol):
    bad, n = run_protocol(state, protocol, "diff_drive", CASES)
    assert n >= (len([c for c in CASES if c["moving"]]) if protocol == "moving_fused" else len(CASES))
    assert not bad, "%d of %d instances:\n%s" % (len(bad), n, "\n".join(bad[:40]))


@pytest.mark.parametrize("protocol", list(PROTOCOLS))
@pytest.mark.parametrize("state", list(STATES))
def test_prologue_sweep_full_body(state, protocol):
    (c,) = [c for c in CASES if c["name"] == FULL_BODY_CASE]
    bad, n = run_protocol(state, protocol, "full_body", [with_v_ref(c, 1.2)])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("protocol", ["still_first", "still_fused"])
@pytest.mark.parametrize("state", [s for s in STATES if s != "single"])
def test_prologue_batch_layout(state, protocol):
    """B = 5, lengths (1, 2, 255, 257, 1025) back to back with per-instance resolution (and v_ref, where the state has a table);
    instances 1 to 3 stand next to the last pose of the slice before theirs and the first pose of the slice after it."""
    steps, advance = PROTOCOLS[protocol]
    table = STATES[state].get("table", False)
    bad = []
    rig = Rig(state)
    try:
        for H in (9, 30):
            chunk = [PR.make_case("layout%d_H%d" % (b, H), "layout", LAYOUT["paths"][b][0], LAYOUT["paths"][b][1], LAYOUT["poses"][b], H=H,
                              expect=LAYOUT["expect"][b], v_ref=LAYOUT["v_ref"][b] if table else LAYOUT["v_ref"][0], dt=LAYOUT["dt"],
                              resolution=LAYOUT["resolution"][b]) for b in range(B)]
            for c, g in zip(chunk, rig.run(chunk, steps, advance)):
                check_still(c, g, steps, bad)
    finally:
        rig.close()
    assert not bad, "\n".join(bad)

"""GPU tests (-m gpu): the disc terms and the grid tap of the batch rollout kernels against their device specs, bit for bit, at
their edges (DESIGN.md sections 10e, 10g, 10h; inputs and expected bits: tests/edge_probe.py, whose docstring has the idea;
tests/test_edge_probe_cpu.py pins the same conditions on the oracle's rollouts and shows every wrong version caught there).

1. One counted state.  Silent, marching instances; term off, discs built from the states the device stored, term on.  The
   term-off costs are +0.0 in every bit; the states of the two runs are bit-equal; every sample of which the spec counts no state
   or one has the spec's cost in every bit (+0.0, fma(w, g_k, 0.0)); the others pass the checkers' bound
   (obstacle_cases.check_penalty / check_moving).  Deep targets count one state, grazing targets one or none and both occur, no
   more than a quarter of an instance's samples count two or more: asserted.
2. Every step at its own time.  One instance per covered step k, one moving disc of 1 mm that is on a state k at step k alone.
3. Grid taps.  One parked instance per probe of grid_probes; cost_on == fma(w, G_ref, cost_off) in every bit with G_ref from
   the reference on the stored states; the two members of every pair across a boundary read different values.  Once more
   with the map derived on the device from an occupancy layer (set_occupancy, R = 0, a checkerboard).

The counts are printed with -s.
"""
import numpy as np
import pytest

import batch_support as BS
import edge_probe as EP
import grid_cases as GC
import grid_reference as GR
import horizon_cases as HC
import obstacle_cases as OC
from batch_support import GRID, MOV, OV, SHIFT
from ccv_mppi_path_tracker_amd import BatchController, capi

pytestmark = pytest.mark.gpu

W = EP.W_EDGE
DISC_CASES = OC.CASES + [("diff_drive", 1000, 15, 5, {}, "plain")]
DISC_IDS = ["%s-K%d-H%d-%s" % (c[0], c[1], c[2], c[5]) for c in DISC_CASES]
FAMILY = {"r4": capi.BATCH_KERNEL_FOUR_WAVE, "r4w": capi.BATCH_KERNEL_FOUR_WAVE | capi.BATCH_KERNEL_WIDE,
          "solo": capi.BATCH_KERNEL_ONE_WAVE, "plain": capi.BATCH_KERNEL_PLAIN}
PLAIN_HEADING = 2.0e5 * np.pi   # outside the fast sin / cos range: the whole batch takes the plain kernel


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(gpu_required):
    capi.load()


def run(bat, inputs):
    """one iteration from the warm start -> per instance the costs and the stored states"""
    x0, dt, xr, yr, yaw0, seeds, nom = inputs
    bat.set_nominal(nom)
    bat.iterate(x0, dt, xr, yr, yaw0, seeds, 0, want_stats=False)
    return [dict(c=bat.read_costs(b), xy=bat.read_candidates(b)) for b in range(bat.B)]


def all_plus_zero(c):
    return not c.view(np.uint64).any()


def check_instance(what, p, x0, dt, discs, vels, targets, off, on):
    """the assertions of test 1 on one instance -> (count 0, count 1, by bound, grazing with g > 0, with g == 0)"""
    assert all_plus_zero(off["c"]), (what, "the silent cost is not +0.0")
    assert on["xy"].tobytes() == off["xy"].tobytes(), what
    T = OC.nstates(p)
    P, ks = on["xy"][:, :T], np.arange(T)
    count, cost = EP.expected_bits(P, ks, x0, dt, discs, vels, W)
    pos, zero = EP.conditions(what, count, targets, len(discs))
    exact = count <= 1
    bad = np.flatnonzero(exact & ~EP.bits_equal(on["c"], np.where(exact, cost, 0.0)))
    n0, n1, rest = int(np.sum(count == 0)), int(np.sum(count == 1)), np.flatnonzero(~exact)
    print("[edges] %s: count 0: %d, count 1: %d (bit for bit; %d differ), by bound: %d; grazing g > 0: %d, g == 0: %d"
          % (what, n0, n1, len(bad), len(rest), pos, zero))
    assert len(bad) == 0, (what, bad[:8], on["c"][bad[:8]], cost[bad[:8]])
    if len(rest):
        near, near_v = EP.near_discs(discs, vels)
        sub_off, sub_on = dict(c=off["c"][rest], xy=off["xy"][rest]), dict(c=on["c"][rest], xy=on["xy"][rest])
        if vels is None:
            OC.check_penalty(what, p, x0, near, W, sub_off, sub_on, share=False)
        else:
            OC.check_moving(what, p, x0, dt, near, near_v, W, sub_off, sub_on, sub_on, share=False)
    return n0, n1, len(rest), pos, zero


# 1. one counted state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,K,H,B,over,fam", DISC_CASES, ids=DISC_IDS)
def test_one_counted_state_is_the_spec_bit_for_bit(model, K, H, B, over, fam, shift, moving):
    p = BS.MODEL_DEFAULTS[model](K, H)
    if over:
        p = p.with_(**over)
    if fam == "solo":
        assert BS.families(model, K, B)[1] == "solo"
    inputs = BS.instance_inputs(p, B)
    if fam == "plain":
        inputs[0][1, 2] += PLAIN_HEADING
    x0, dt = inputs[0], inputs[1]
    plist, ns, T = EP.march_params(p, B), EP.disc_counts(B), OC.nstates(p)
    bat = BatchController(plist, B, min_shift=shift)
    off = run(bat, inputs)
    discs, vels, targets = [], [], []
    for b in range(B):
        n = ns[b % len(ns)]
        P = off[b]["xy"][:, :T]
        d, v, t = EP.single_state_discs(P[:64] if fam == "solo" else P, x0[b], dt[b], n, moving, lead=EP.lead_of(B, n, shift) if n in (1, 3) else None)
        discs.append(d)
        vels.append(v)
        targets.append(t)
    bat.set_obstacles(discs, W, velocities=vels if moving else None)
    on = run(bat, inputs)
    assert bat.last_kernel() == FAMILY[fam] | (MOV if moving else OV) | (SHIFT if shift else 0)
    bat.close()
    tot = np.zeros(5, dtype=np.int64)
    for b in range(B):
        what = "%s K=%d H=%d %s%s%s b=%d n=%d" % (model, K, H, fam, " shift" if shift else "", " moving" if moving else "", b, len(discs[b]))
        tot += check_instance(what, plist[b], x0[b], dt[b], discs[b], vels[b] if moving else None, targets[b], off[b], on[b])
    print("[edges] %s K=%d H=%d %s%s%s: count 0: %d, count 1: %d, by bound: %d, grazing g > 0: %d, g == 0: %d"
          % ((model, K, H, fam, " shift" if shift else "", " moving" if moving else "") + tuple(tot)))
    assert tot[3] >= 1 and tot[4] >= 1, "the grazing targets do not show both outcomes"


# 2. every step at its own time ---------------------------------------------------------------------------------------------
STEP_CASES = [("diff_drive", H) for H in (9, 10, 15, 17, 26)] + [("full_body", H) for H in (10, 15)]


@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,H", STEP_CASES, ids=["%s-H%d" % c for c in STEP_CASES])
def test_every_step_is_charged_at_its_own_time(model, H, shift):
    K = 128
    p = BS.MODEL_DEFAULTS[model](K, H)
    T = OC.nstates(p)
    B = T   # instance k carries the disc of step k (a disc on state 0 or 1 counts for every sample: it needs an instance of its own)
    assert BS.families(model, K, B)[1] == "r4"
    inputs = BS.instance_inputs(p, B)
    x0, dt = inputs[0], inputs[1]
    plist = EP.march_params(p, B)
    bat = BatchController(plist, B, min_shift=shift)
    off = run(bat, inputs)
    aim = [(7 * k + 3) % K for k in range(T)]
    made = [EP.step_disc(off[k]["xy"][aim[k], k], k, dt[k], k) for k in range(T)]
    discs, vels = [m[0][None, :] for m in made], [m[1][None, :] for m in made]
    bat.set_obstacles(discs, W, velocities=vels)
    on = run(bat, inputs)
    assert bat.last_kernel() == capi.BATCH_KERNEL_FOUR_WAVE | MOV | (SHIFT if shift else 0)
    bat.close()
    reached = set()
    for k in range(T):
        what = "%s H=%d%s step %d" % (model, H, " shift" if shift else "", k)
        assert all_plus_zero(off[k]["c"]) and on[k]["xy"].tobytes() == off[k]["xy"].tobytes(), what
        count, cost = EP.expected_bits(on[k]["xy"][:, :T], np.arange(T), x0[k], dt[k], discs[k], vels[k], W)
        assert count[aim[k]] == 1 and count.max() == 1, (what, int(count[aim[k]]), int(count.max()))
        assert np.all(EP.bits_equal(on[k]["c"], cost)), (what, on[k]["c"][aim[k]], cost[aim[k]])
        if on[k]["c"][aim[k]] > 0.0:
            reached.add((k // HC.K_TU, k % HC.K_TU))
    print("[edges] %s H=%d%s: (block, i) reached: %s" % (model, H, " shift" if shift else "", sorted(reached)))
    assert reached == {(b, i) for b, width in enumerate(HC.consumer_widths(model, H)) for i in range(width)}


# 3. grid taps at cell boundaries ---------------------------------------------------------------------------------------------
MAPS = EP.probe_maps()
W_GRID = 0.01    # (not dyadic: the product rounds)
GRID_FORMS = [("diff_drive", "r4"), ("diff_drive", "solo"), ("diff_drive", "plain"), ("full_body", "r4"), ("full_body", "plain")]
# (full body beyond one workgroup per CU has no one-wave grid form: tests/test_gpu_batch_grid.py)


def grid_run(model, fam, shift, g, set_map):
    """parked instances on the probes of g, term off and on -> (p, probes, names, pairs, off, on); the assertions on codes,
    parking and the identity made on the way"""
    K, H = 64, 15
    p = EP.parked(BS.MODEL_DEFAULTS[model](K, H))
    probes, names, pairs = EP.grid_probes(g)
    N = len(probes)
    B = 5 * BS.cus() + 1 if fam == "solo" else N
    inputs = EP.probe_inputs(p, probes[np.arange(B) % N], extra_heading=PLAIN_HEADING if fam == "plain" else None)
    B = len(inputs[1])
    assert BS.families(model, K, B)[1] == ("solo" if fam == "solo" else "r4")
    bat = BatchController(p, B, min_shift=shift)
    off = run(bat, inputs)
    g = set_map(bat, B) or g
    on = run(bat, inputs)
    assert bat.last_kernel() == FAMILY[fam] | GRID | (SHIFT if shift else 0)
    bat.close()
    T = GR.n_covered(model, H)
    for b in range(B):
        what = "%s %s%s probe %s" % (model, fam, " shift" if shift else "", names[b % N] if b < N or fam == "solo" else "extra")
        assert EP.is_parked(off[b]["xy"][:, :T], inputs[0][b]), what
        GC.check_identity(what, p, g, W_GRID, off[b], on[b], conditions=False)
    v, _, _ = GR.lookup(g, np.array([on[b]["xy"][0, 0, 0] for b in range(N)]), np.array([on[b]["xy"][0, 0, 1] for b in range(N)]))
    for lo, hi, axis, m in pairs:
        assert v[lo] != v[hi], (names[lo], names[hi], v[lo], v[hi])
    print("[edges] grid %s %s%s: %d probes on %d instances, %d pairs across a boundary" % (model, fam, " shift" if shift else "", N, B, len(pairs)))
    return g, on


@pytest.mark.parametrize("m", range(len(MAPS)), ids=["dyadic", "tenth", "far"])
@pytest.mark.parametrize("shift", [False, True], ids=["plain_w", "shift"])
@pytest.mark.parametrize("model,fam", GRID_FORMS, ids=["%s-%s" % f for f in GRID_FORMS])
def test_grid_taps_at_cell_boundaries(model, fam, shift, m):
    g = MAPS[m]
    grid_run(model, fam, shift, g, lambda bat, B: bat.set_grids([g.as_tuple()], np.zeros(B, dtype=np.int32), W_GRID))


def test_costmap_cells_meet_the_same_taps():
    """the second map once more, its cells derived on the device from an occupancy layer: a checkerboard, R = 0 -- an occupied
    cell costs profile[0], a free one free_value, so the two sides of every inner cell edge differ as well"""
    g0 = MAPS[1]
    occ = np.where((np.arange(g0.nx)[None, :] + np.arange(g0.ny)[:, None]) % 2 == 1, 255, 0).astype(np.uint8)
    lethal, free = 7.0, 1.5
    want = np.where(occ >= 128, lethal, free).astype(np.float32)

    def set_map(bat, B):
        bat.set_occupancy([(occ, (g0.ox, g0.oy), g0.resolution, float(g0.outside), 128)], (0, np.float32([lethal]), free),
                          np.zeros(B, dtype=np.int32), W_GRID)
        (cells, origin, resolution, outside), = bat.get_grids()[0]
        assert cells.tobytes() == want.tobytes() and (origin, resolution, outside) == ((g0.ox, g0.oy), g0.resolution, float(g0.outside))
        return GR.Grid(cells, origin, resolution, outside)

    grid_run("diff_drive", "r4", True, g0, set_map)

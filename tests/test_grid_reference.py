"""CPU tests of tests/grid_reference.py, the checker of the occupancy-grid term: the numpy backend and
the exact-rational backend agree in every bit over a battery of edge cases, ten wrong versions of the spec each differ from
it on some case of that battery, and the maps the GPU tests place (map_ahead) meet their coverage conditions on the oracle's
Philox-mode rollouts of the GPU tests' own configurations."""
import math

import numpy as np
import pytest

import batch_support as BS
import grid_cases as GC
import grid_reference as GR
import obstacle_cases as OC

NAN, INF = float("nan"), float("inf")


def ulp_up(v):
    return float(np.nextafter(v, INF))


def ulp_down(v):
    return float(np.nextafter(v, -INF))


def battery():
    """[(name, grid, states [n][2], n_covered)]: one sample each"""
    rng = np.random.default_rng(7)
    out = []
    # a 5 x 3 map of non-integer float32 cells (a float32 sum of them rounds), origin off zero, a resolution whose reciprocal
    # rounds, outside != 0
    cells = (0.1 + 0.37 * np.arange(15)).astype(np.float32).reshape(3, 5)
    g = GR.Grid(cells, (0.7, -1.3), 0.3, 4.25)
    w, h = g.nx * g.resolution, g.ny * g.resolution
    inner = [(g.ox + (i + 0.5) * g.resolution, g.oy + (j + 0.5) * g.resolution) for j in range(g.ny) for i in range(g.nx)]
    out.append(("every cell centre", g, inner, len(inner)))
    # cell edges and both sides of every map edge by one ulp
    edge = []
    for i in range(g.nx + 1):
        x = g.ox + i * g.resolution
        edge += [(x, g.oy + 0.4), (ulp_up(x), g.oy + 0.4), (ulp_down(x), g.oy + 0.4)]
    for j in range(g.ny + 1):
        y = g.oy + j * g.resolution
        edge += [(g.ox + 0.8, y), (g.ox + 0.8, ulp_up(y)), (g.ox + 0.8, ulp_down(y))]
    for x in (g.ox, g.ox + w):
        for y in (g.oy, g.oy + h):
            edge += [(x, y), (ulp_up(x), ulp_up(y)), (ulp_down(x), ulp_down(y)), (ulp_up(x), ulp_down(y)), (ulp_down(x), ulp_up(y))]
    out.append(("edges by one ulp", g, edge, len(edge)))
    # multiples of the resolution from the origin: states on cell edges, as the sum of origin and multiple rounds them
    mult = [(g.ox + i * g.resolution, g.oy + (i % g.ny) * g.resolution) for i in range(0, 40)]
    out.append(("multiples of the resolution", g, mult, len(mult)))
    # origin zero, resolution 0.7, x = i * 0.7: 7, 14, 23, 28, 45 ... are where (x / res) and (x * RN(1 / res)) fall on different
    # sides of the cell edge (every cell of the row a distinct value)
    gd = GR.Grid(1.0 + np.arange(100, dtype=np.float32).reshape(1, 100), (0.0, 0.0), 0.7, 4.25)
    out.append(("reciprocal against division", gd, [(i * 0.7, 0.35) for i in range(1, 90)], 89))
    out.append(("not numbers", g, [(NAN, g.oy + 0.1), (g.ox + 0.1, NAN), (NAN, NAN), (INF, g.oy + 0.1), (-INF, g.oy + 0.1),
                                   (g.ox + 0.1, INF), (g.ox + 0.1, -INF), (INF, -INF), (g.ox + 0.1, g.oy + 0.1)], 9))
    out.append(("random around the map", g, [(g.ox + w * (1.6 * rng.random() - 0.3), g.oy + h * (1.6 * rng.random() - 0.3))
                                             for _ in range(200)], 200))
    # origin at zero: negative zero, fx exactly 0 and exactly nx (resolution a power of two: every product is exact)
    g0 = GR.Grid(1.0 + np.arange(12, dtype=np.float32).reshape(3, 4), (0.0, 0.0), 0.25, -7.0)
    out.append(("zeros and exact edges", g0, [(-0.0, -0.0), (0.0, 0.0), (-0.0, 0.3), (0.3, -0.0), (1.0, 0.1), (0.1, 0.75),
                                              (ulp_down(1.0), ulp_down(0.75)), (-5e-324, 0.1), (0.1, -5e-324), (0.99, 0.74)], 10))
    # nx = 1, ny = 1, nx != ny
    g1 = GR.Grid(np.float32([[3.0], [5.0], [9.0]]), (-0.2, 0.1), 0.37, 2.0)
    out.append(("nx = 1", g1, [(-0.2 + 0.37 * a, 0.1 + 0.37 * b) for a in (-0.5, 0.0, 0.5, 1.0, 1.5) for b in (-0.5, 0.5, 1.5, 2.5, 3.5)], 25))
    g2 = GR.Grid(np.float32([[3.0, 5.0, 9.0, 17.0]]), (-0.2, 0.1), 0.37, 2.0)
    out.append(("ny = 1", g2, [(-0.2 + 0.37 * a, 0.1 + 0.37 * b) for a in (-0.5, 0.5, 1.5, 2.5, 3.5, 4.5) for b in (-0.5, 0.0, 0.5, 1.0, 1.5)], 30))
    # full body: the last two states do not count -- and would, here, change the sum
    fb = inner[:6] + [inner[7], inner[11]]
    out.append(("full body's H - 2", g, fb, GR.n_covered("full_body", len(fb))))
    # a far origin: the subtraction rounds
    gf = GR.Grid(cells, (1234567.891, -7654321.123), 0.05, 4.25)
    out.append(("far origin", gf, [(gf.ox + 0.25 * rng.random(), gf.oy + 0.15 * rng.random()) for _ in range(100)], 100))
    return out


BATTERY = battery()
W = 0.1          # a weight whose products round
COST_REST = 3.7


def spec(g, P, n):
    G = float(GR.grid_sum(g, np.asarray(P, dtype=np.float64)[None, :n])[0])
    return G, GR.fma(W, G, COST_REST)


@pytest.mark.parametrize("name,g,P,n", BATTERY, ids=[b[0] for b in BATTERY])
def test_the_two_backends_agree_in_every_bit(name, g, P, n):
    P = np.asarray(P, dtype=np.float64)
    v, inside, idx = GR.lookup(g, P[:, 0], P[:, 1])
    for k in range(len(P)):
        ve, ine, idxe = GR.lookup_exact(g, P[k, 0], P[k, 1])
        assert (np.float32(ve).tobytes(), bool(ine), int(idxe)) == (v[k].tobytes(), bool(inside[k]), int(idx[k])), (name, k, P[k])
    G = GR.grid_sum(g, P[None, :n])[0]
    assert np.float64(G).tobytes() == np.float64(GR.grid_sum_exact(g, P[:n])).tobytes(), name


def test_the_battery_has_what_it_says():
    by = {b[0]: b for b in BATTERY}
    _, g, P, n = by["edges by one ulp"]
    _, inside, _ = GR.lookup(g, *np.asarray(P).T)
    assert inside.any() and (~inside).any()
    _, g0, P0, _ = by["zeros and exact edges"]
    v, inside, idx = GR.lookup(g0, *np.asarray(P0).T)
    assert inside[:4].all() and idx[0] == 0                      # -0.0 >= 0: cell 0
    assert not inside[4] and not inside[5]                       # fx == nx, fy == ny: outside
    assert inside[6] and idx[6] == g0.nx * g0.ny - 1             # one ulp below both: the last cell
    assert not inside[7] and not inside[8]                       # the smallest negative number: outside
    _, g, P, _ = by["not numbers"]
    v, inside, _ = GR.lookup(g, *np.asarray(P).T)
    assert not inside[:8].any() and inside[8] and all(x == g.outside for x in v[:8])


def test_fma_is_one_rounding():
    a, b, c = 0.1, 3.0, -0.30000000000000004   # a * b rounds to -c; the exact product does not
    assert a * b + c == 0.0 and GR.fma(a, b, c) != 0.0
    assert GR.fma(0.0, 5.0, 2.5) == 2.5 and GR.fma(2.0, 3.0, 1.0) == 7.0
    assert math.isnan(GR.fma(1.0, NAN, 1.0)) and GR.fma(1.0, 2.0, INF) == INF
    assert GR.fma(1e308, 10.0, 0.0) == INF


# ---- wrong versions: each must differ from the spec on some case of the battery ----------------------------------------------
def wrong_sum(g, P, n, variant):
    """G, cost of one sample by a version of the spec with one mistake (plain float64 / float32 numpy scalars)"""
    G = np.float32(0.0) if variant == "float32 accumulation" else 0.0
    cost = COST_REST
    count = len(P) if variant == "last two full-body states included" else n
    for k in range(count):
        x, y = float(P[k][0]), float(P[k][1])
        with np.errstate(invalid="ignore", over="ignore"):
            dx = np.float64(x) - (0.0 if variant == "origin not subtracted" else g.ox)
            dy = np.float64(y) - (0.0 if variant == "origin not subtracted" else g.oy)
            if variant == "division by the resolution":
                fx, fy = dx / g.resolution, dy / g.resolution
            else:
                fx, fy = dx * g.inv, dy * g.inv
        hi_x = fx <= g.nx if variant == "<= at the upper edge" else fx < g.nx
        hi_y = fy <= g.ny if variant == "<= at the upper edge" else fy < g.ny
        inside = bool(fx >= 0 and hi_x and fy >= 0 and hi_y)
        if inside:
            if variant == "rounding to nearest":
                ix, iy = int(np.rint(fx)), int(np.rint(fy))
            else:
                ix, iy = int(fx), int(fy)
            if variant == "x and y transposed":
                idx = ix * g.nx + iy
            elif variant == "row pitch ny":
                idx = iy * g.ny + ix
            else:
                idx = iy * g.nx + ix
            v = g.cells.reshape(-1)[idx % g.cells.size]   # (a wrong index stays an index)
        else:
            v = np.float32(0.0) if variant == "outside read as 0" else g.outside
        if variant == "float32 accumulation":
            G = np.float32(G + np.float32(v))
        else:
            G = G + float(v)
        if variant == "weight applied per state":
            cost = GR.fma(W, float(v), cost)
    if variant != "weight applied per state":
        cost = GR.fma(W, float(G), cost)
    return float(G), cost


WRONG = ["x and y transposed", "row pitch ny", "rounding to nearest", "<= at the upper edge", "origin not subtracted",
         "division by the resolution", "outside read as 0", "last two full-body states included", "weight applied per state",
         "float32 accumulation"]


def test_the_restatement_without_a_mistake_is_the_spec():
    for name, g, P, n in BATTERY:
        G, cost = wrong_sum(g, P, n, None)
        Gs, cs = spec(g, P, n)
        assert (np.float64(G).tobytes(), np.float64(cost).tobytes()) == (np.float64(Gs).tobytes(), np.float64(cs).tobytes()), name


@pytest.mark.parametrize("variant", WRONG)
def test_a_wrong_version_differs_on_some_case(variant):
    hits = []
    for name, g, P, n in BATTERY:
        _, cost = wrong_sum(g, P, n, variant)
        _, cs = spec(g, P, n)
        if np.float64(cost).tobytes() != np.float64(cs).tobytes():
            hits.append(name)
    print("%s: differs on %s" % (variant, hits))
    assert hits, variant


# ---- the GPU tests' maps on the oracle's rollouts ---------------------------------------------------------------------------
def test_the_gpu_tests_maps_meet_their_conditions_on_the_oracles_rollouts():
    """every instance with a map: >= 25 % of the covered states in bounds, >= 5 % out of bounds, >= 50 distinct cells hit"""
    seen = set()
    for model, K, H, B, over, fam in GC.CASES + [GC.PLAIN_CASE]:
        K = min(K, 1000)   # (the one-wave case differs from the first in K alone: the fan is the same)
        if (model, K, H, tuple(over.items())) in seen:
            continue
        seen.add((model, K, H, tuple(over.items())))
        p = BS.MODEL_DEFAULTS[model](K, H)
        if over:
            p = p.with_(**over)
        inputs = GC.grid_inputs(p, B)
        maps, map_of, _ = GC.maps_for(p, inputs)
        x0, dt, xr, yr, yaw0, seeds, nom = inputs
        for b in range(B):
            if map_of[b] < 0:
                continue
            P = OC.oracle_states(p, x0[b], dt[b], nom[b], seeds[b], 0)
            share_in, share_out, cells = GR.coverage(maps[map_of[b]], P)
            print("%s K=%d H=%d %s b=%d: in %.2f out %.2f cells %d" % (model, K, H, over, b, share_in, share_out, cells))
            assert share_in >= 0.25 and share_out >= 0.05 and cells >= 50, (model, K, H, over, b, share_in, share_out, cells)

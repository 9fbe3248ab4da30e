"""B independent MPPI problems in one launch: the batch handle of the C ABI (ccv_mppi_batch_*, include/ccv_mppi.h).

Every array carries the instance as its first axis.  Instance b computes what an MPPIController with instance b's parameters
computes for the same inputs and warm start; all compute happens in libccv_mppi_hip.so.
"""
import ctypes as C
from dataclasses import replace

import numpy as np

from . import capi
from .controller import MPPIError, make_config
from .configs import MPPIParams


def _is_1d(a):
    try:
        return np.asarray(a, dtype=np.float64).ndim == 1
    except (TypeError, ValueError):
        return False


# the fields every instance of a batch shares (they fix the layout and the kernels); the rest may differ per instance
SHARED_FIELDS = ("model", "horizon", "roll_off", "steer_off", "num_samples")


def check_shared(seq, first=None):
    """ValueError unless every MPPIParams of `seq` agrees with `first` (default: seq[0]) in SHARED_FIELDS."""
    first = seq[0] if first is None else first
    for b, p in enumerate(seq):
        for f in SHARED_FIELDS:
            if getattr(p, f) != getattr(first, f):
                raise ValueError("params[%d].%s = %r differs from the batch's %r (shared by every instance)"
                                 % (b, f, getattr(p, f), getattr(first, f)))


def pack_obstacles(discs, weight, batch):
    """The arguments of ccv_mppi_batch_set_obstacles from `batch` arrays of (ox, oy, r) rows (instance b's discs; an empty
    sequence or None: none) and a weight per instance (or one for all): xyr [B][max_n][3] (rows past an instance's count
    zero), n [B] int32, max_n = the largest count, weight [B].  ValueError for a wrong number of instances, rows that are not
    triples or more than capi.MAX_OBSTACLES discs; the values themselves are the library's to refuse."""
    discs = list(discs)
    if len(discs) != int(batch):
        raise ValueError("obstacles: expected %d arrays of (ox, oy, r) rows, got %d" % (int(batch), len(discs)))
    rows = []
    for b, d in enumerate(discs):
        a = np.zeros((0, 3)) if d is None else np.asarray(d, dtype=np.float64)
        if a.size == 0:
            a = np.zeros((0, 3))
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("obstacles[%d]: expected shape (n, 3), got %s" % (b, a.shape))
        if a.shape[0] > capi.MAX_OBSTACLES:
            raise ValueError("obstacles[%d]: %d discs, at most %d" % (b, a.shape[0], capi.MAX_OBSTACLES))
        rows.append(a)
    n = np.ascontiguousarray([a.shape[0] for a in rows], dtype=np.int32)
    max_n = int(n.max()) if len(rows) else 0
    xyr = np.zeros((int(batch), max_n, 3))
    for b, a in enumerate(rows):
        xyr[b, :a.shape[0]] = a
    w = capi.as_f64(np.broadcast_to(np.asarray(weight, dtype=np.float64), (int(batch),)))
    return xyr, n, max_n, w


def pack_velocities(velocities, batch, counts=None):
    """The arguments of ccv_mppi_batch_set_obstacle_velocities from `batch` arrays of (vx, vy) rows (instance b's discs in the
    order of pack_obstacles; an empty sequence or None: none): vxy [B][max_n][2] (rows past an instance's count zero) and
    max_n.  counts: the instances' disc counts, when the caller wants them checked.  ValueError for a wrong number of
    instances, rows that are not pairs, more than capi.MAX_OBSTACLES rows or a count that differs."""
    velocities = list(velocities)
    if len(velocities) != int(batch):
        raise ValueError("velocities: expected %d arrays of (vx, vy) rows, got %d" % (int(batch), len(velocities)))
    rows = []
    for b, v in enumerate(velocities):
        a = np.zeros((0, 2)) if v is None else np.asarray(v, dtype=np.float64)
        if a.size == 0:
            a = np.zeros((0, 2))
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("velocities[%d]: expected shape (n, 2), got %s" % (b, a.shape))
        if a.shape[0] > capi.MAX_OBSTACLES:
            raise ValueError("velocities[%d]: %d rows, at most %d" % (b, a.shape[0], capi.MAX_OBSTACLES))
        if counts is not None and a.shape[0] != int(counts[b]):
            raise ValueError("velocities[%d]: %d rows for %d discs" % (b, a.shape[0], int(counts[b])))
        rows.append(a)
    max_n = max([a.shape[0] for a in rows], default=0)
    vxy = np.zeros((int(batch), max_n, 2))
    for b, a in enumerate(rows):
        vxy[b, :a.shape[0]] = a
    return vxy, max_n


def pack_exposed(sizes, dx, dy, exposed, fill=0):
    """The `exposed` buffer of ccv_mppi_batch_roll_occupancy_enqueue: per entry the row strip and then the column strip, tightly
    packed.  sizes: (nx, ny) per entry; exposed: (row_strip [min(|dy|, ny)][nx], col_strip [ny - min(|dy|, ny)][min(|dx|, nx)])
    per entry, each in ascending new-frame iy and ix (an empty strip may be None), or None for an entry whose exposed cells all
    become `fill`."""
    if len(exposed) != len(sizes):
        raise ValueError("exposed: expected %d pairs of strips, got %d" % (len(sizes), len(exposed)))
    parts = []
    for i, ((nx, ny), pair) in enumerate(zip(sizes, exposed)):
        ax, ay = min(abs(int(dx[i])), nx), min(abs(int(dy[i])), ny)
        if pair is None:
            parts.append(np.full(ay * nx + (ny - ay) * ax, int(fill), dtype=np.uint8))
            continue
        rows, cols = pair
        for name, strip, shape in (("row", rows, (ay, nx)), ("column", cols, (ny - ay, ax))):
            strip = np.zeros(shape, dtype=np.uint8) if strip is None and 0 in shape else np.ascontiguousarray(strip, dtype=np.uint8)
            if strip.size == 0:
                strip = strip.reshape(shape)
            if strip.shape != shape:
                raise ValueError("entry %d: the %s strip must be %s, got %s" % (i, name, shape, strip.shape))
            parts.append(strip.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint8)


def scan_cells(geometry, sensor_xy, sensor_yaw, ranges, angle_min, angle_increment, range_min, range_max):
    """One entry of BatchController.scan_occupancy from a planar range scan (a sensor_msgs/LaserScan): (sensor_cell (sx, sy),
    ends int32 [n][2], hits uint8 [n]).  geometry: the map's entry of get_occupancy().  Beam k leaves the sensor at world
    position sensor_xy under the angle sensor_yaw + angle_min + k * angle_increment.  Points go to cells by the grid term's
    formula with floor in place of the truncation: cell = floor((p - origin) * (1.0 / resolution)), so a point left of or below
    the map gets a negative cell.  A range that is NaN or below range_min drops the beam; a range >= range_max (+inf included)
    is a miss: the ray ends at range_max with hit = 0; a ray of more than capi.SCAN_MAX_REACH cells is cut at its own cell
    SCAN_MAX_REACH and becomes a miss.  The sensor's cell is returned as it is: the call refuses one outside the map."""
    (ox, oy), resolution = geometry[0], geometry[1]
    inv = 1.0 / float(resolution)
    r = np.asarray(ranges, dtype=np.float64).reshape(-1)
    ang = float(sensor_yaw) + float(angle_min) + np.arange(r.size, dtype=np.float64) * float(angle_increment)
    with np.errstate(invalid="ignore"):
        keep = ~np.isnan(r) & ~(r < float(range_min))
        miss = r >= float(range_max)
    r, ang, hits = np.where(miss, float(range_max), r)[keep], ang[keep], ~miss[keep]
    sx, sy = int(np.floor((float(sensor_xy[0]) - ox) * inv)), int(np.floor((float(sensor_xy[1]) - oy) * inv))
    ex = np.floor(((float(sensor_xy[0]) + r * np.cos(ang)) - ox) * inv).astype(np.int64)
    ey = np.floor(((float(sensor_xy[1]) + r * np.sin(ang)) - oy) * inv).astype(np.int64)
    # a ray beyond the reach ends in its own cell i = SCAN_MAX_REACH (the closed form of the call)
    dx, dy = ex - sx, ey - sy
    a, b = np.maximum(np.abs(dx), np.abs(dy)), np.minimum(np.abs(dx), np.abs(dy))
    far = a > capi.SCAN_MAX_REACH
    minor = (2 * capi.SCAN_MAX_REACH * b + a) // np.maximum(2 * a, 1)
    xmajor = np.abs(dx) >= np.abs(dy)
    ex = np.where(far, sx + np.sign(dx) * np.where(xmajor, capi.SCAN_MAX_REACH, minor), ex)
    ey = np.where(far, sy + np.sign(dy) * np.where(xmajor, minor, capi.SCAN_MAX_REACH), ey)
    ends = np.ascontiguousarray(np.stack([ex, ey], axis=1), dtype=np.int32).reshape(-1, 2)
    return (sx, sy), ends, np.ascontiguousarray(hits & ~far, dtype=np.uint8)


def beam_fan(n, reach_cells, phase=0.0):
    """The beam table of BatchController.resident_sense for a sensor that looks all round: int32 [n][2], beam k's end offset
    (rint(reach_cells * cos(t)), rint(reach_cells * sin(t))) with t = phase + 2 pi k / n -- the rint of a circle's points, so no
    component exceeds reach_cells in magnitude.  ValueError unless n >= 1 and 0 <= reach_cells <= capi.SCAN_MAX_REACH."""
    n, reach = int(n), float(reach_cells)
    if n < 1 or not 0.0 <= reach <= capi.SCAN_MAX_REACH:
        raise ValueError("beam_fan: need n >= 1 and 0 <= reach_cells <= %d" % capi.SCAN_MAX_REACH)
    t = float(phase) + 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.ascontiguousarray(np.stack([np.rint(reach * np.cos(t)), np.rint(reach * np.sin(t))], axis=1), dtype=np.int32)


def goal_cells(geometry, xy):
    """Goal cells for BatchController.resident_plan: int32 [n][2], the cell of each point xy [n][2] of a map with
    geometry = ((origin_x, origin_y), resolution, nx, ny) by the grid term's formula -- f = (p - origin) * (1 / resolution), one
    subtraction and one multiplication, truncated -- clamped to the map: a point outside it gets the nearest border cell (a NaN
    coordinate cell 0)."""
    (ox, oy), resolution, nx, ny = geometry
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    inv = 1.0 / float(resolution)
    out = np.empty(xy.shape, dtype=np.int32)
    for k, (o, n) in enumerate(((float(ox), int(nx)), (float(oy), int(ny)))):
        f = (xy[:, k] - o) * inv
        out[:, k] = np.trunc(np.clip(np.where(np.isnan(f), 0.0, f), 0.0, n - 1)).astype(np.int32)
    return np.ascontiguousarray(out)


def plan_multiplier(cells, gain, max_penalty):
    """The multipliers of BatchController.resident_set_plan_penalty in numpy: int32, the shape of `cells`, m = 1 + q with
    t = float32(cell) * float32(gain) (one fp32 multiplication) and q = 0 where not t > 0 (zero, negative, NaN), max_penalty where
    t >= max_penalty, else t truncated.  A step of a weighted plan out of cell c costs 5 * m(c) straight and 7 * m(c) diagonal."""
    max_penalty = int(max_penalty)
    if not 0 <= max_penalty <= capi.PLAN_MAX_PENALTY:
        raise ValueError("plan_multiplier: max_penalty outside [0, %d]" % capi.PLAN_MAX_PENALTY)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = np.asarray(cells, dtype=np.float32) * np.float32(gain)
        positive = t > 0
    q = np.trunc(np.minimum(np.where(positive, t, np.float32(0)), np.float32(max_penalty)))
    return np.ascontiguousarray(1 + q.astype(np.int32))


def follow_shift(geometry, pose_xy, margin, max_step):
    """The decision of BatchController.resident_follow in numpy, for callers who drive the host prologue and therefore know the
    pose (they roll with roll_occupancy): int32 [n][2], the cells (dx, dy) the window of a map with geometry = ((origin_x,
    origin_y), resolution, nx, ny) moves for each pose pose_xy [n][2].  Per axis e = floor((p - origin) * (1 / resolution)) -
    n // 2 and d = 0 where |e| <= margin, else e clamped to [-max_step, max_step]; (0, 0) for a pose that is not finite or
    2^30 cells or more from the origin.  (The limit of 2^30 accumulated cells is the roll's own check.)"""
    (ox, oy), resolution, nx, ny = geometry
    xy = np.asarray(pose_xy, dtype=np.float64).reshape(-1, 2)
    inv = 1.0 / float(resolution)
    f = np.stack([(xy[:, 0] - float(ox)) * inv, (xy[:, 1] - float(oy)) * inv], axis=1)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(f) < 2.0 ** 30, axis=1)
    e = np.floor(np.where(ok[:, None], f, 0.0)).astype(np.int64) - np.array([int(nx) // 2, int(ny) // 2], dtype=np.int64)
    d = np.where(np.abs(e) <= int(margin), 0, np.clip(e, -int(max_step), int(max_step)))
    return np.ascontiguousarray(np.where(ok[:, None], d, 0), dtype=np.int32)


def inflation_profile(radius_m, resolution, kind="linear", lethal=1.0, inscribed=None, inscribed_m=0.0, free_value=0.0, scaling=10.0):
    """(R, profile float32 [R * R + 1], free_value) for BatchController.set_occupancy: the cost of a cell by the squared distance
    D2, in cells, from its centre to the centre of the nearest occupied cell, built on the host -- the device only looks it up.
    R = ceil(radius_m / resolution) cells.  With d = sqrt(D2) * resolution: d = 0 -> lethal; d <= inscribed_m -> inscribed
    (default: lethal); inscribed_m < d <= radius_m -> by `kind`: "step": inscribed; "linear": from inscribed at inscribed_m down to
    free_value at radius_m; "exponential": inscribed * exp(-scaling * (d - inscribed_m)) (nav2's inflation layer, scaling in
    1 / m); d > radius_m -> free_value.  ValueError for an unknown kind, a radius of more than capi.INFLATE_MAX_RADIUS cells or
    an inscribed_m above radius_m."""
    radius_m, resolution, inscribed_m = float(radius_m), float(resolution), float(inscribed_m)
    if not (resolution > 0.0 and radius_m >= 0.0 and 0.0 <= inscribed_m <= radius_m):
        raise ValueError("inflation_profile: need resolution > 0 and 0 <= inscribed_m <= radius_m")
    R = int(np.ceil(radius_m / resolution - 1e-9))
    if R > capi.INFLATE_MAX_RADIUS:
        raise ValueError("inflation_profile: %d cells, at most %d" % (R, capi.INFLATE_MAX_RADIUS))
    inscribed = float(lethal if inscribed is None else inscribed)
    d = np.sqrt(np.arange(R * R + 1, dtype=np.float64)) * resolution
    if kind == "step":
        f = np.full_like(d, inscribed)
    elif kind == "linear":
        f = inscribed + (free_value - inscribed) * (d - inscribed_m) / max(radius_m - inscribed_m, np.finfo(float).tiny)
    elif kind == "exponential":
        f = inscribed * np.exp(-float(scaling) * (d - inscribed_m))
    else:
        raise ValueError("inflation_profile: kind must be 'step', 'linear' or 'exponential', not %r" % (kind,))
    f = np.where(d <= inscribed_m, inscribed, f)
    f = np.where(d > radius_m, float(free_value), f)
    f[0] = float(lethal)
    return R, np.ascontiguousarray(f, dtype=np.float32), float(free_value)


class BatchController:
    """`batch` controllers on one device: one MPPIParams shared by all, or a sequence of `batch` MPPIParams that agree in
    SHARED_FIELDS (per-instance sigma, lambda, v_ref, bounds and weights; K = num_samples per instance).  min_shift: the
    underflow-safe weights from the first iteration on (set_min_shift)."""

    def __init__(self, params, batch, device=0, num_samples=None, no_state_store=False, min_shift=False):
        seq = None
        if not isinstance(params, MPPIParams):
            seq = list(params)
            if len(seq) != int(batch):
                raise ValueError("params: expected one MPPIParams or %d, got %d" % (int(batch), len(seq)))
            check_shared(seq)
            params = seq[0]
        self.lib = capi.load()
        self.params = params
        self.params_list = [params] * int(batch)
        self.B = int(batch)
        self.K = int(num_samples if num_samples is not None else params.num_samples)
        self.H = params.horizon
        self.udim = params.udim
        self.nstate = params.nstate
        self.device = int(device)
        self._plan_dims = None   # (nx, ny) per map for _default_sweeps; set_grids / set_occupancy forget it
        self.no_state_store = bool(no_state_store)
        self._h = capi._H()
        cfg = make_config(params, device, 0, False, no_state_store, self.K)
        rc = self.lib.ccv_mppi_batch_create(C.byref(cfg), self.B, C.byref(self._h))
        if rc != capi.OK:
            self._h = capi._H()
            raise MPPIError(rc, "ccv_mppi_batch_create failed (bad arguments, or no usable MI355X/HIP device) -- there is no CPU fallback")
        if seq is not None:
            self.set_params(seq)
        if min_shift:
            self.set_min_shift(True)

    # ---- plumbing ----
    def _check(self, rc):
        if rc != capi.OK:
            msg = self.lib.ccv_mppi_batch_last_error(self._h)
            raise MPPIError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.ccv_mppi_batch_destroy(self._h)
            self._h = capi._H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self._check(self.lib.ccv_mppi_batch_set_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._check(self.lib.ccv_mppi_batch_synchronize(self._h))

    def last_kernel(self):
        """capi.BATCH_KERNEL_* of the last iteration (| BATCH_KERNEL_WIDE for the wide-turn form), -1 before the first."""
        return self.lib.ccv_mppi_batch_last_kernel(self._h)

    # ---- per-instance parameters (ccv_mppi_batch_set_params) ----
    def set_params(self, seq):
        """seq: B MPPIParams (instance b's sigma, lambda, v_ref, bounds, weights, resolution), or None: every instance back to
        the creation parameters and the shared kernels.  Disagreeing SHARED_FIELDS raise ValueError before the library is
        called.  Flushes a pending resident update; warm starts, paths and poses stay."""
        if seq is None:
            self._check(self.lib.ccv_mppi_batch_set_params(self._h, None))
            self.params_list = [self.params] * self.B
            return
        seq = list(seq)
        if len(seq) != self.B:
            raise ValueError("params: expected %d MPPIParams, got %d" % (self.B, len(seq)))
        check_shared(seq, self.params)
        cfgs = (capi.Config * self.B)(*[make_config(p, self.device, 0, False, self.no_state_store, self.K) for p in seq])
        self._check(self.lib.ccv_mppi_batch_set_params(self._h, cfgs))
        self.params_list = seq

    def get_params(self):
        """The B effective MPPIParams, as the library holds them (dt and resolution: the host side's)."""
        cfgs = (capi.Config * self.B)()
        self._check(self.lib.ccv_mppi_batch_get_params(self._h, cfgs))
        out = []
        for p, c in zip(self.params_list, cfgs):
            ud = p.udim
            out.append(replace(p, control_noise=c.control_noise, lam=c.lam, v_ref=c.v_ref,
                               u_min=tuple(c.u_min[:ud]), u_max=tuple(c.u_max[:ud]), path_weight=c.path_weight,
                               v_weight=c.v_weight, zmp_weight=c.zmp_weight, roll_v_weight=c.roll_v_weight,
                               back_weight=c.back_weight, yaw_weight=c.yaw_weight))
        return out

    # ---- underflow-safe weights (ccv_mppi_batch_set_min_shift) ----
    def set_min_shift(self, on=True):
        """on: every instance weighs its samples relative to its own smallest cost, w = exp(-(c - min c) / lambda_b) -- a finite
        cost always gives a finite u*; off: back to the reference's weights.  Flushes a pending resident update; warm starts,
        paths, poses and per-instance parameters stay."""
        self._check(self.lib.ccv_mppi_batch_set_min_shift(self._h, 1 if on else 0))

    def get_min_shift(self):
        return bool(self.lib.ccv_mppi_batch_get_min_shift(self._h))

    # ---- per-instance disc obstacles (ccv_mppi_batch_set_obstacles) ----
    def set_obstacles(self, discs, weight=0.0, velocities=None):
        """discs: B arrays of (ox, oy, r) rows in world coordinates (an instance without discs: an empty one), or None: the term
        off and the kernels that ran before; weight: one value or [B], >= 0.  The cost of every state the path term covers gains
        weight_b * max(max_j(r_j^2 - |p - o_j|^2), 0).  A weight that matters needs set_min_shift(True).  velocities: B arrays of
        (vx, vy) rows, one per disc (set_obstacle_velocities), or None: the discs stand still.  Flushes a pending resident
        update; warm starts, paths, poses and per-instance parameters stay."""
        if discs is None:
            self._check(self.lib.ccv_mppi_batch_set_obstacles(self._h, None, None, 0, None))
            return
        xyr, n, max_n, w = pack_obstacles(discs, weight, self.B)
        if velocities is not None:
            vxy, vmax = pack_velocities(velocities, self.B, n)   # (checked before the discs change)
        self._check(self.lib.ccv_mppi_batch_set_obstacles(self._h, capi.dptr(xyr), n.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          max_n, capi.dptr(w)))
        if velocities is not None:
            self._check(self.lib.ccv_mppi_batch_set_obstacle_velocities(self._h, capi.dptr(vxy), vmax))

    def set_obstacle_velocities(self, velocities):
        """velocities: B arrays of (vx, vy) rows in world coordinates, one per disc of set_obstacles (constant over the
        horizon: state k is charged against the disc at o + v k dt), or None: back to the static term and its bits.  Any table,
        one of zeros too, runs the MOVING kernels.  Flushes a pending resident update."""
        if velocities is None:
            self._check(self.lib.ccv_mppi_batch_set_obstacle_velocities(self._h, None, 0))
            return
        vxy, max_n = pack_velocities(velocities, self.B)
        self._check(self.lib.ccv_mppi_batch_set_obstacle_velocities(self._h, capi.dptr(vxy), max_n))

    def get_obstacle_velocities(self):
        """List of B arrays [n_b][2] as the library holds them; zeros while no velocities are set."""
        n = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ccv_mppi_batch_get_obstacles(self._h, None, n.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          capi.MAX_OBSTACLES, None))
        vxy = np.zeros((self.B, capi.MAX_OBSTACLES, 2))
        self._check(self.lib.ccv_mppi_batch_get_obstacle_velocities(self._h, capi.dptr(vxy), capi.MAX_OBSTACLES))
        return [vxy[b, :n[b]].copy() for b in range(self.B)]

    def get_obstacles(self):
        """(list of B arrays [n_b][3], weight [B]) as the library holds them; empty arrays and zeros while the term is off."""
        n = np.zeros(self.B, dtype=np.int32)
        w = np.zeros(self.B)
        xyr = np.zeros((self.B, capi.MAX_OBSTACLES, 3))
        self._check(self.lib.ccv_mppi_batch_get_obstacles(self._h, capi.dptr(xyr), n.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          capi.MAX_OBSTACLES, capi.dptr(w)))
        return [xyr[b, :n[b]].copy() for b in range(self.B)], w

    def set_grids(self, maps, map_of=None, weight=0.0):
        """maps: a list of (cells[ny][nx] float32, (origin_x, origin_y), resolution, outside), or None: the term off and the
        kernels that ran before; map_of: [B] index of the instance's map, -1 for none; weight: one value or [B], >= 0.  Every
        state the path term covers reads the cell it lies in (cells[int(fy)][int(fx)], f = (p - origin) * (1 / resolution);
        `outside` where there is none) and the cost gains weight_b * their sum.  Flushes a pending resident update; warm
        starts, paths, poses, per-instance parameters and discs stay."""
        self._plan_dims = None
        if maps is None or len(maps) == 0:
            self._check(self.lib.ccv_mppi_batch_set_grids(self._h, None, 0, None, None))
            return
        rows = (capi.Grid * len(maps))()
        keep = []
        for m, (cells, origin, resolution, outside) in enumerate(maps):
            cells = np.ascontiguousarray(cells, dtype=np.float32)
            if cells.ndim != 2:
                raise ValueError("map %d: cells must be [ny][nx]" % m)
            keep.append(cells)
            rows[m] = capi.Grid(float(origin[0]), float(origin[1]), float(resolution), float(outside), cells.shape[1], cells.shape[0],
                                cells.ctypes.data_as(C.POINTER(C.c_float)))
        mo = np.ascontiguousarray(np.broadcast_to(np.asarray(map_of, dtype=np.int32), (self.B,)))
        w = capi.as_f64(np.broadcast_to(np.asarray(weight, dtype=np.float64), (self.B,)))
        self._check(self.lib.ccv_mppi_batch_set_grids(self._h, rows, len(maps), mo.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(w)))

    def get_grids(self):
        """(maps, map_of [B], weight [B]) as the library holds them, maps a list of (cells[ny][nx] float32, (origin_x, origin_y),
        resolution, outside) with the cells read back from the device; ([], all -1, zeros) while the term is off."""
        n = C.c_int32(0)
        mo = np.zeros(self.B, dtype=np.int32)
        w = np.zeros(self.B)
        self._check(self.lib.ccv_mppi_batch_get_grids(self._h, None, 0, C.byref(n), mo.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(w)))
        rows = (capi.Grid * max(n.value, 1))()
        self._check(self.lib.ccv_mppi_batch_get_grids(self._h, rows, n.value, None, None, None))
        maps = []
        for m in range(n.value):
            g = rows[m]
            cells = np.empty((g.ny, g.nx), dtype=np.float32)
            self._check(self.lib.ccv_mppi_batch_read_grid_cells(self._h, m, cells.ctypes.data_as(C.POINTER(C.c_float))))
            maps.append((cells, (g.origin_x, g.origin_y), g.resolution, g.outside))
        return maps, mo, w

    # ---- costmaps inflated on the device (ccv_mppi_batch_set_occupancy) ----
    def set_occupancy(self, maps, inflation=None, map_of=None, weight=0.0):
        """maps: a list of (cells[ny][nx] uint8, (origin_x, origin_y), resolution, outside, threshold), or None: the grid term off;
        inflation: one (R, profile[R * R + 1], free_value) per map (inflation_profile), or one for all; map_of, weight: as
        set_grids.  The float cells the grid term reads are derived on the device: a cell whose nearest occupied cell
        (cells >= threshold) is at squared distance D2 <= R * R costs profile[D2], every other cell free_value.  Takes the place
        of set_grids' maps (and a later set_grids takes the place of these); get_grids returns the derived cells.  Flushes a
        pending resident update."""
        self._plan_dims = None
        if maps is None or len(maps) == 0:
            self._check(self.lib.ccv_mppi_batch_set_occupancy(self._h, None, None, 0, None, None))
            return
        if len(inflation) == 3 and np.isscalar(inflation[0]):
            inflation = [inflation] * len(maps)
        if len(inflation) != len(maps):
            raise ValueError("inflation: expected one (R, profile, free_value) or %d, got %d" % (len(maps), len(inflation)))
        rows, infl, keep = (capi.Occupancy * len(maps))(), (capi.Inflation * len(maps))(), []
        for m, ((cells, origin, resolution, outside, threshold), (R, profile, free_value)) in enumerate(zip(maps, inflation)):
            cells = np.ascontiguousarray(cells, dtype=np.uint8)
            profile = np.ascontiguousarray(profile, dtype=np.float32)
            if cells.ndim != 2:
                raise ValueError("map %d: cells must be [ny][nx]" % m)
            if profile.shape != (int(R) * int(R) + 1,):
                raise ValueError("map %d: profile must have R * R + 1 = %d entries, got %s" % (m, int(R) * int(R) + 1, profile.shape))
            keep += [cells, profile]
            rows[m] = capi.Occupancy(float(origin[0]), float(origin[1]), float(resolution), float(outside), cells.shape[1], cells.shape[0],
                                     int(threshold), cells.ctypes.data_as(C.POINTER(C.c_uint8)))
            infl[m] = capi.Inflation(int(R), float(free_value), profile.ctypes.data_as(C.POINTER(C.c_float)))
        mo = np.ascontiguousarray(np.broadcast_to(np.asarray(map_of, dtype=np.int32), (self.B,)))
        w = capi.as_f64(np.broadcast_to(np.asarray(weight, dtype=np.float64), (self.B,)))
        self._check(self.lib.ccv_mppi_batch_set_occupancy(self._h, rows, infl, len(maps), mo.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(w)))

    def update_occupancy(self, map, x0, y0, patch2d):
        """Map `map`'s occupancy cells [y0 : y0 + h, x0 : x0 + w] become patch2d [h][w] uint8, and the float cells within R of them
        are derived again, in stream order: a step enqueued before this call reads the old map, every step enqueued after it
        the new one.  No synchronisation; patch2d may be reused as soon as the call returns.  At most
        capi.OCC_PATCH_MAX_CELLS cells."""
        patch = np.ascontiguousarray(patch2d, dtype=np.uint8)
        if patch.ndim != 2:
            raise ValueError("patch2d must be [h][w]")
        self._check(self.lib.ccv_mppi_batch_update_occupancy_enqueue(self._h, int(map), int(x0), int(y0), patch.shape[1], patch.shape[0],
                                                                      patch.ctypes.data_as(C.POINTER(C.c_uint8))))

    def roll_occupancy(self, maps, dx, dy, exposed=None, fill=0):
        """The windows of the maps `maps` (each at most once) move by (dx[i], dy[i]) whole cells, in stream order and in two launches
        for all of them: new[iy][ix] = old[iy + dy][ix + dx] where that lies inside the map, the origin moves by (dx, dy) *
        resolution (formed from the accumulated cell count, so it never drifts), and the float cells are what set_occupancy of
        the new layer would derive.  exposed: None -- every exposed cell becomes `fill` -- or per map a pair (row_strip
        [min(|dy|, ny)][nx], col_strip [ny - min(|dy|, ny)][min(|dx|, nx)]) of uint8 in the new frame, or None for a map whose
        exposed cells become `fill` (pack_exposed).  No
        synchronisation, except that the handle's first roll allocates the second set of layers and synchronises once (a roll by
        zeros primes it); the arguments may be reused when the call returns."""
        maps = np.ascontiguousarray(np.atleast_1d(maps), dtype=np.int32)
        dx = np.ascontiguousarray(np.broadcast_to(np.asarray(dx, dtype=np.int32), maps.shape))
        dy = np.ascontiguousarray(np.broadcast_to(np.asarray(dy, dtype=np.int32), maps.shape))
        buf = None
        if exposed is not None:
            geo = self.get_occupancy()
            if any(not 0 <= int(m) < len(geo) for m in maps):
                raise ValueError("a map out of range")
            buf = pack_exposed([(geo[int(m)][3], geo[int(m)][4]) for m in maps], dx, dy, exposed, fill)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_roll_occupancy_enqueue(
            self._h, len(maps), maps.ctypes.data_as(ip), dx.ctypes.data_as(ip), dy.ctypes.data_as(ip),
            buf.ctypes.data_as(C.POINTER(C.c_uint8)) if buf is not None else None, int(fill)))

    def scan_occupancy(self, maps, sensor_cells, ends, hits, clear=0, mark=255):
        """Range scans traced into the maps `maps` (each at most once), in stream order and in two launches for all of them.  Per
        entry: sensor_cells[i] = (sx, sy), the sensor's cell, inside the map; ends[i] int32 [n_i][2], the rays' end cells (they
        may lie outside); hits[i] [n_i], non-zero where the ray ended on something (scan_cells makes all three from a
        LaserScan).  Every cell a ray passes through, from the sensor's cell up to but not including the end cell, becomes
        `clear`; then every hit's end cell becomes `mark` -- marks win over clears whatever the order of rays and entries --
        and the float cells are what set_occupancy of the new layer would derive.  Cells are those of the map's current
        (rolled) frame.  No synchronisation; the arguments may be reused when the call returns."""
        maps = np.ascontiguousarray(np.atleast_1d(maps), dtype=np.int32)
        if not (len(sensor_cells) == len(ends) == len(hits) == len(maps)):
            raise ValueError("scan_occupancy: expected %d sensor cells, end arrays and hit arrays" % len(maps))
        sensors = np.ascontiguousarray(np.asarray(sensor_cells, dtype=np.int32).reshape(len(maps), 2))
        ends = [np.asarray(e, dtype=np.int32).reshape(-1, 2) for e in ends]
        hits = [np.asarray(h).reshape(-1) != 0 for h in hits]
        if any(len(e) != len(h) for e, h in zip(ends, hits)):
            raise ValueError("scan_occupancy: an entry's ends and hits differ in length")
        n_rays = np.ascontiguousarray([len(e) for e in ends], dtype=np.int32)
        end_xy = np.ascontiguousarray(np.concatenate(ends + [np.zeros((0, 2), dtype=np.int32)]), dtype=np.int32)
        hit = np.ascontiguousarray(np.concatenate(hits + [np.zeros(0, dtype=bool)]), dtype=np.uint8)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_scan_occupancy_enqueue(
            self._h, len(maps), maps.ctypes.data_as(ip), sensors.ctypes.data_as(ip), n_rays.ctypes.data_as(ip), end_xy.ctypes.data_as(ip),
            hit.ctypes.data_as(C.POINTER(C.c_uint8)), int(clear), int(mark)))

    def get_occupancy(self):
        """A list of ((origin_x, origin_y), resolution, outside, nx, ny, threshold, R, free_value) per map as the library holds
        them; [] unless occupancy is set.  (map_of and weight: get_grids.)"""
        n = C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_get_occupancy(self._h, None, None, 0, C.byref(n)))
        rows, infl = (capi.Occupancy * max(n.value, 1))(), (capi.Inflation * max(n.value, 1))()
        self._check(self.lib.ccv_mppi_batch_get_occupancy(self._h, rows, infl, n.value, None))
        return [((g.origin_x, g.origin_y), g.resolution, g.outside, g.nx, g.ny, g.threshold, f.radius, f.free_value)
                for g, f in zip(rows[:n.value], infl[:n.value])]

    def read_occupancy(self, map):
        """cells[ny][nx] uint8 of map `map`, read back from the device; synchronises."""
        geo = self.get_occupancy()
        if not 0 <= int(map) < max(len(geo), 1):
            raise ValueError("map %d out of range" % int(map))
        ny, nx = (geo[int(map)][4], geo[int(map)][3]) if geo else (1, 1)   # (no occupancy: the library refuses)
        out = np.empty((ny, nx), dtype=np.uint8)
        self._check(self.lib.ccv_mppi_batch_read_occupancy(self._h, int(map), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- range sensors simulated on the device (ccv_mppi_batch_set_world, _resident_sense_enqueue) ----
    def set_world(self, cells, threshold=1, origin=(0.0, 0.0), resolution=1.0, anchors=None, max_beams=capi.SENSE_MAX_BEAMS):
        """The ground-truth world the resident robots' beams are cast through: cells [ny][nx] uint8 (occupied: >= threshold),
        or None: no world.  anchors [n_maps][2] int32: the world cell that coincided with each occupancy map's cell (0, 0) when
        set_occupancy was called (the maps must have the world's resolution bit for bit).  max_beams: the most beams a
        resident_sense call may carry.  Needs set_occupancy; a later set_occupancy or set_grids drops the world.  Flushes a
        pending resident update."""
        if cells is None:
            self._check(self.lib.ccv_mppi_batch_set_world(self._h, None, None, 0))
            return
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        if cells.ndim != 2:
            raise ValueError("set_world: cells must be [ny][nx]")
        anchors = np.ascontiguousarray(np.asarray(anchors, dtype=np.int32).reshape(-1, 2))
        n_maps = len(self.get_occupancy())
        if n_maps and len(anchors) != n_maps:
            raise ValueError("set_world: expected %d anchors, got %d" % (n_maps, len(anchors)))
        row = capi.Occupancy(float(origin[0]), float(origin[1]), float(resolution), 0.0, cells.shape[1], cells.shape[0], int(threshold),
                             cells.ctypes.data_as(C.POINTER(C.c_uint8)))
        self._check(self.lib.ccv_mppi_batch_set_world(self._h, C.byref(row), anchors.ctypes.data_as(C.POINTER(C.c_int32)), int(max_beams)))

    def get_world(self):
        """((origin_x, origin_y), resolution, nx, ny, threshold, anchors int32 [n_maps][2], max_beams) as the library holds
        them; MPPIError (capi.ERR_STATE) while no world is set."""
        row, mb = capi.Occupancy(), C.c_int32(0)
        n_maps = len(self.get_occupancy())
        anchors = np.zeros((n_maps, 2), dtype=np.int32)
        self._check(self.lib.ccv_mppi_batch_get_world(self._h, C.byref(row), anchors.ctypes.data_as(C.POINTER(C.c_int32)), n_maps, C.byref(mb)))
        return (row.origin_x, row.origin_y), row.resolution, row.nx, row.ny, row.threshold, anchors, mb.value

    def read_world(self):
        """cells [ny][nx] uint8 of the world, read back from the device; synchronises."""
        row = capi.Occupancy()
        self._check(self.lib.ccv_mppi_batch_get_world(self._h, C.byref(row), None, 0, None))
        out = np.empty((row.ny, row.nx), dtype=np.uint8)
        self._check(self.lib.ccv_mppi_batch_read_world(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def update_world(self, x0, y0, patch2d):
        """The world's cells [y0 : y0 + h, x0 : x0 + w] become patch2d [h][w] uint8, in stream order: a resident_sense enqueued
        before this call reads the old world, every one enqueued after it the new one.  No synchronisation."""
        patch = np.ascontiguousarray(patch2d, dtype=np.uint8)
        if patch.ndim != 2:
            raise ValueError("patch2d must be [h][w]")
        self._check(self.lib.ccv_mppi_batch_update_world_enqueue(self._h, int(x0), int(y0), patch.shape[1], patch.shape[0],
                                                                  patch.ctypes.data_as(C.POINTER(C.c_uint8))))

    def resident_sense(self, instances, beams, clear=0, mark=255):
        """The instances `instances` (each at most once, each on a map of its own) sense, in stream order and in two launches for
        all of them: from the world cell its resident pose lies in, each casts the beams `beams` int32 [n][2] (end offsets in
        cells, world-aligned: beam_fan) through the world.  A beam clears its map's cells up to the first occupied world cell
        and marks that cell, or clears up to its end cell and marks nothing; marks come after all clears; the float cells are
        what set_occupancy of the new layer would derive.  A robot outside the world senses nothing.  No synchronisation; the
        arguments may be reused when the call returns."""
        inst = np.ascontiguousarray(np.atleast_1d(instances), dtype=np.int32)
        beams = np.ascontiguousarray(np.asarray(beams, dtype=np.int32).reshape(-1, 2))
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_resident_sense_enqueue(self._h, len(inst), inst.ctypes.data_as(ip), len(beams), beams.ctypes.data_as(ip),
                                                                    int(clear), int(mark)))

    def resident_read_sense(self):
        """(first int32 [B][max_beams], sensor_cell int32 [B][2]): per instance the blocked cell index of every beam of its last
        sensing (-1: not blocked, or nothing sensed) and the world cell it sensed from ((-1, -1): nothing sensed); synchronises."""
        mb = C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_get_world(self._h, None, None, 0, C.byref(mb)))
        first = np.empty((self.B, mb.value), dtype=np.int32)
        cell = np.empty((self.B, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_resident_read_sense(self._h, first.ctypes.data_as(ip), cell.ctypes.data_as(ip)))
        return first, cell

    # ---- warm starts [B][H-1][u_dim] ----
    def set_nominal(self, u):
        u = capi.as_f64(u, (self.B, self.H - 1, self.udim))
        self._check(self.lib.ccv_mppi_batch_set_nominal(self._h, capi.dptr(u)))

    def get_nominal(self):
        u = np.empty((self.B, self.H - 1, self.udim))
        self._check(self.lib.ccv_mppi_batch_get_nominal(self._h, capi.dptr(u)))
        return u

    # ---- whole iteration of every instance ----
    def _inputs(self, x0, dt, x_ref, y_ref, yaw_ref0, seed):
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim != 2 or x0.shape[0] != self.B or x0.shape[1] > 5:
            raise ValueError("x0: expected shape (%d, <= 5), got %s" % (self.B, x0.shape))
        x = np.zeros((self.B, 5))
        x[:, :x0.shape[1]] = x0
        d = capi.as_f64(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.B,)))
        xr, yr = capi.as_f64(x_ref, (self.B, self.H)), capi.as_f64(y_ref, (self.B, self.H))
        yw = capi.as_f64(np.broadcast_to(np.asarray(yaw_ref0, dtype=np.float64), (self.B,)))
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, dtype=np.uint64), (self.B,)))
        return x, d, xr, yr, yw, sd

    def iterate(self, x0, dt, x_ref, y_ref, yaw_ref0, seed, iteration, want_stats=True):
        """x0 [B][nstate], dt / yaw_ref0 / seed [B] (or one value for all), x_ref / y_ref [B][H] -> u* [B][H-1][u_dim]
        (and a list of B capi.Stats)."""
        x, d, xr, yr, yw, sd = self._inputs(x0, dt, x_ref, y_ref, yaw_ref0, seed)
        u = np.empty((self.B, self.H - 1, self.udim))
        st = (capi.Stats * self.B)()
        self._check(self.lib.ccv_mppi_batch_iterate(self._h, capi.dptr(x), capi.dptr(d), capi.dptr(xr), capi.dptr(yr),
                                                    capi.dptr(yw), sd.ctypes.data_as(C.POINTER(C.c_uint64)), int(iteration),
                                                    capi.dptr(u), st if want_stats else None))
        return (u, list(st)) if want_stats else u

    def iterate_enqueue(self, x0, dt, x_ref, y_ref, yaw_ref0, seed, iteration):
        x, d, xr, yr, yw, sd = self._inputs(x0, dt, x_ref, y_ref, yaw_ref0, seed)
        self._check(self.lib.ccv_mppi_batch_iterate_enqueue(self._h, capi.dptr(x), capi.dptr(d), capi.dptr(xr), capi.dptr(yr),
                                                            capi.dptr(yw), sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                            int(iteration)))

    # ---- per-instance read-back of the last iteration ----
    def read_costs(self, instance, first=0, count=None):
        count = self.K - first if count is None else count
        out = np.empty(count)
        self._check(self.lib.ccv_mppi_batch_read_costs(self._h, int(instance), int(first), int(count), capi.dptr(out)))
        return out

    def read_weights(self, instance, first=0, count=None):
        count = self.K - first if count is None else count
        out = np.empty(count)
        self._check(self.lib.ccv_mppi_batch_read_weights(self._h, int(instance), int(first), int(count), capi.dptr(out)))
        return out

    def read_candidates(self, instance, first=0, count=None, stride=1):
        count = self.K if count is None else count
        out = np.empty((count, self.H, 2))
        self._check(self.lib.ccv_mppi_batch_read_candidates(self._h, int(instance), int(first), int(count), int(stride),
                                                            capi.dptr(out)))
        return out

    # ---- what a node publishes per robot, for every instance at once (ccv_mppi_batch_read_best_candidates / _optimal_paths) ----
    def read_best_candidates(self, count, with_paths=True):
        """The `count` lowest-cost samples of every instance of the last tick: (idx int32 [B, count], cost [B, count],
        xy [B, count, H, 2] or None without with_paths).  Costs ascend, ties go to the lower sample index, NaN costs come last:
        the order of np.lexsort((np.arange(K), cost)).  Selected, ordered and gathered on the device; does not flush a pending
        resident update.  count <= min(K, capi.BEST_MAX)."""
        count = int(count)
        n = max(count, 0)
        idx = np.empty((self.B, n), dtype=np.int32)
        cost = np.empty((self.B, n))
        xy = np.empty((self.B, n, self.H, 2)) if with_paths else None
        self._check(self.lib.ccv_mppi_batch_read_best_candidates(self._h, count, idx.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(cost),
                                                                 capi.dptr(xy) if with_paths else None))
        return idx, cost, xy

    def read_optimal_paths(self):
        """[B, H-1, 3]: the plant model rolled through every instance's u* from the pose and dt of the last tick, row i =
        (x, y, yaw) before control step i -- plant_step() H-1 times, on the device.  Flushes a pending resident update."""
        out = np.empty((self.B, self.H - 1, 3))
        self._check(self.lib.ccv_mppi_batch_read_optimal_paths(self._h, capi.dptr(out)))
        return out

    # ---- device-resident closed loop of every instance (ccv_mppi_batch_resident_*) ----
    def resident_set_paths(self, paths, resolution=None):
        """paths: B (path_x, path_y) pairs, or one pair for every instance; resolution: one value or [B] (default: each
        instance's parameters' resolution)."""
        if len(paths) == 2 and _is_1d(paths[0]) and _is_1d(paths[1]):
            paths = [paths] * self.B
        if len(paths) != self.B:
            raise ValueError("paths: expected %d (path_x, path_y) pairs, got %d" % (self.B, len(paths)))
        xs, ys = [], []
        for b, (px, py) in enumerate(paths):
            px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
            if px.ndim != 1 or px.shape != py.shape or px.size < 1:
                raise ValueError("path %d: path_x and path_y must be non-empty 1-D arrays of one length" % b)
            xs.append(px)
            ys.append(py)
        n = np.ascontiguousarray([len(px) for px in xs], dtype=np.int32)
        if resolution is None:
            plist = getattr(self, "params_list", None) or [self.params] * self.B
            resolution = [p.resolution for p in plist]
        res = resolution
        res = capi.as_f64(np.broadcast_to(np.asarray(res, dtype=np.float64), (self.B,)))
        px, py = capi.as_f64(np.concatenate(xs)), capi.as_f64(np.concatenate(ys))
        self._check(self.lib.ccv_mppi_batch_resident_set_paths(self._h, capi.dptr(px), capi.dptr(py),
                                                               n.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(res)))

    def resident_set_poses(self, states, seeds):
        """states [B][nstate] (x, y, yaw[, roll, pitch]); seeds [B] (or one value): every instance's noise key."""
        st = np.asarray(states, dtype=np.float64)
        if st.ndim != 2 or st.shape[0] != self.B or not 3 <= st.shape[1] <= 5:
            raise ValueError("states: expected shape (%d, 3..5), got %s" % (self.B, st.shape))
        x = np.zeros((self.B, 5))
        x[:, :st.shape[1]] = st
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (self.B,)))
        self._check(self.lib.ccv_mppi_batch_resident_set_poses(self._h, capi.dptr(x), sd.ctypes.data_as(C.POINTER(C.c_uint64))))

    def resident_step_enqueue(self, dt, iteration, advance=True):
        """One tick of every instance, no host data: (advance) pose += plant(u*[b][0]) -> window -> MPPI iteration."""
        self._check(self.lib.ccv_mppi_batch_resident_step_enqueue(self._h, float(dt), int(iteration), 1 if advance else 0))

    def resident_read(self):
        """(states [B][nstate], current_index [B], x_ref [B][H], y_ref [B][H], yaw_ref0 [B], steps); synchronises."""
        st = np.zeros((self.B, 5))
        idx = np.zeros(self.B, dtype=np.int32)
        xr, yr, yaw0 = np.zeros((self.B, self.H)), np.zeros((self.B, self.H)), np.zeros(self.B)
        steps = C.c_int64()
        self._check(self.lib.ccv_mppi_batch_resident_read(self._h, capi.dptr(st), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          capi.dptr(xr), capi.dptr(yr), capi.dptr(yaw0), C.byref(steps)))
        return st[:, :self.nstate].copy(), idx, xr, yr, yaw0, steps.value

    def resident_read_trace(self, instance, max_rows=None):
        """Instance `instance`'s poses of the last ticks, oldest first: rows (x, y, yaw, roll, pitch, current_index)."""
        max_rows = capi.BATCH_TRACE_ROWS if max_rows is None else int(max_rows)
        rows = np.zeros((max(max_rows, 0), 6))
        n = C.c_int32()
        self._check(self.lib.ccv_mppi_batch_resident_read_trace(self._h, int(instance), max_rows, capi.dptr(rows), C.byref(n)))
        return rows[:n.value].copy()

    # ---- paths planned on the device (ccv_mppi_batch_resident_set_plan, _plan_enqueue; include/ccv_mppi_plan.h) ----
    def resident_set_plan(self, capacity, keep_fields=False):
        """capacity: one value or [B], the most poses a planned path of the instance may have (0: the instance does not plan, at
        most capi.PLAN_MAX_POSES), or None: planning off, the paths stay as they are.  keep_fields: every planning instance's
        distance field is kept for resident_read_plan_field.  After resident_set_paths, which also turns planning off; every
        path keeps its bits.  Flushes a pending resident update and synchronises."""
        if capacity is None:
            self._check(self.lib.ccv_mppi_batch_resident_set_plan(self._h, None, 0))
            return
        cap = np.ascontiguousarray(np.broadcast_to(np.asarray(capacity, dtype=np.int32), (self.B,)))
        self._check(self.lib.ccv_mppi_batch_resident_set_plan(self._h, cap.ctypes.data_as(C.POINTER(C.c_int32)), 1 if keep_fields else 0))

    def resident_get_plan(self):
        """(capacity int32 [B], keep_fields) as the library holds them; MPPIError (capi.ERR_STATE) while planning is off."""
        cap, keep = np.zeros(self.B, dtype=np.int32), C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_resident_get_plan(self._h, cap.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(keep)))
        return cap, bool(keep.value)

    def resident_plan(self, instances, goals, lethal, max_sweeps=None):
        """The instances `instances` (each at most once) plan, in stream order and in one launch for all of them: from the cell
        of its own map its resident pose lies in, each gets the path of cell centres that descends the map's distance field to
        its goal cell goals [n][2] (goal_cells), over the cells whose value is <= lethal, 8-connected without corner cutting.
        max_sweeps: the most relaxation sweeps (default: the largest nx * ny + 1 of the named instances' maps, which is always
        enough).  The outcome: resident_read_plan.  No synchronisation; the arguments may be reused when the call returns."""
        inst = np.ascontiguousarray(np.atleast_1d(instances), dtype=np.int32)
        goals = np.ascontiguousarray(np.asarray(goals, dtype=np.int32).reshape(-1, 2))
        if len(goals) != len(inst):
            raise ValueError("resident_plan: expected %d goals, got %d" % (len(inst), len(goals)))
        if max_sweeps is None:
            max_sweeps = self._default_sweeps(inst)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_resident_plan_enqueue(self._h, len(inst), inst.ctypes.data_as(ip), goals.ctypes.data_as(ip),
                                                                   float(lethal), int(max_sweeps)))

    def _default_sweeps(self, inst):
        """the largest nx * ny + 1 of the named instances' maps (the sizes never change, so no synchronisation is needed)"""
        n = C.c_int32(0)
        mo = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ccv_mppi_batch_get_grids(self._h, None, 0, C.byref(n), mo.ctypes.data_as(C.POINTER(C.c_int32)), None))
        if self._plan_dims is None or len(self._plan_dims) != n.value:
            rows = (capi.Grid * max(n.value, 1))()
            self._check(self.lib.ccv_mppi_batch_get_grids(self._h, rows, n.value, None, None, None))
            self._plan_dims = [(rows[m].nx, rows[m].ny) for m in range(n.value)]
        named = [mo[b] for b in inst if 0 <= b < self.B and mo[b] >= 0]
        return min(max([self._plan_dims[m][0] * self._plan_dims[m][1] + 1 for m in named] or [1]), capi.PLAN_MAX_FIELD)

    def resident_read_plan(self):
        """(status [B], poses [B], start_cell [B][2], start_dist [B], sweeps [B]), int32, of every instance's last plan: status a
        capi.PLAN_* value (0: never planned), poses the cells the descent visited (0 without one), start_cell the cell the pose
        lay in ((-1, -1): in none), start_dist the field's value there (-1: no converged field); synchronises."""
        out = [np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32), np.zeros((self.B, 2), dtype=np.int32),
               np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)]
        self._check(self.lib.ccv_mppi_batch_resident_read_plan(self._h, *[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in out]))
        return tuple(out)

    def resident_read_plan_field(self, instance, shape):
        """uint16 [ny][nx] (shape = (ny, nx) of the instance's map): the distance field of the instance's last plan -- 65535 on
        blocked cells, 0 on the goal, 65533 where the goal is not reached within 65532; synchronises.  MPPIError
        (capi.ERR_STATE) without keep_fields or while the last plan's status is not OK, TRUNCATED or UNREACHABLE."""
        out = np.empty((int(shape[0]), int(shape[1])), dtype=np.uint16)
        self._check(self.lib.ccv_mppi_batch_resident_read_plan_field(self._h, int(instance), out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def resident_read_path(self, instance):
        """(path_x, path_y) of the instance as the device holds it now, planned or set; synchronises."""
        n = C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_resident_read_path(self._h, int(instance), 0, None, None, C.byref(n)))
        x, y = np.empty(n.value), np.empty(n.value)
        self._check(self.lib.ccv_mppi_batch_resident_read_path(self._h, int(instance), n.value, capi.dptr(x), capi.dptr(y), C.byref(n)))
        return x[:n.value], y[:n.value]

    # ---- traversal weights of the planned paths (ccv_mppi_batch_resident_set_plan_penalty; include/ccv_mppi_plan_cost.h) ----
    def resident_set_plan_penalty(self, gain, max_penalty):
        """Every later resident_plan / resident_plan_goals charges a step out of cell c 5 * m(c) straight and 7 * m(c) diagonal,
        m = plan_multiplier(cell, gain, max_penalty): paths keep clear of costly cells where a detour is cheaper.  gain finite and
        >= 0, max_penalty in [0, capi.PLAN_MAX_PENALTY]; (0, 0), which every resident_set_plan starts with: the unweighted plan.
        After resident_set_plan (MPPIError, capi.ERR_STATE, before); host state only, no synchronisation."""
        self._check(self.lib.ccv_mppi_batch_resident_set_plan_penalty(self._h, float(np.float32(gain)), int(max_penalty)))

    def resident_get_plan_penalty(self):
        """(gain, max_penalty) as the library holds them; MPPIError (capi.ERR_STATE) while planning is off."""
        gain, max_penalty = C.c_float(0.0), C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_resident_get_plan_penalty(self._h, C.byref(gain), C.byref(max_penalty)))
        return gain.value, max_penalty.value

    # ---- costmaps that follow their robots (ccv_mppi_batch_resident_set_follow, _follow_enqueue; include/ccv_mppi_follow.h) ----
    def resident_set_follow(self, on=True):
        """The occupancy maps follow their robots from now on (resident_follow), or no longer.  While on, the device holds every
        map's frame: roll_occupancy is refused (capi.ERR_STATE), resident_sense and resident_plan work in the frame as the
        device has it, get_grids / get_occupancy synchronise to show it.  Needs set_occupancy; a later set_occupancy or
        set_grids turns it off.  Flushes a pending resident update and synchronises."""
        self._check(self.lib.ccv_mppi_batch_resident_set_follow(self._h, 1 if on else 0))

    def resident_get_follow(self):
        on = C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_resident_get_follow(self._h, C.byref(on)))
        return bool(on.value)

    def resident_follow(self, instances, margin, max_step, fill=0):
        """The maps of the instances `instances` (each at most once, each on a map of its own) are re-centred on their robots'
        resident poses, in stream order and in two launches for all of them, decided on the device (follow_shift is the same
        decision in numpy): per axis the window moves by d = 0 while the robot's cell is within `margin` cells of the centre
        cell, else by the distance to it clamped to `max_step`; exposed cells become `fill`, the float cells are what
        set_occupancy of the new layer would derive.  The outcome: resident_read_follow.  No synchronisation; the arguments
        may be reused when the call returns."""
        inst = np.ascontiguousarray(np.atleast_1d(instances), dtype=np.int32)
        self._check(self.lib.ccv_mppi_batch_resident_follow_enqueue(self._h, len(inst), inst.ctypes.data_as(C.POINTER(C.c_int32)), int(margin),
                                                                     int(max_step), int(fill)))

    def resident_read_follow(self):
        """(status int32 [n_maps], shift int32 [n_maps][2], offset int64 [n_maps][2], origin [n_maps][2]): per map the
        capi.FOLLOW_* status (0: never followed) and the cells moved by its last resident_follow, the cells moved since
        set_occupancy and the origin now; synchronises."""
        n = C.c_int32(0)
        self._check(self.lib.ccv_mppi_batch_get_occupancy(self._h, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        status, shift = np.zeros(m, dtype=np.int32), np.zeros((m, 2), dtype=np.int32)
        offset, origin = np.zeros((m, 2), dtype=np.int64), np.zeros((m, 2))
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.ccv_mppi_batch_resident_read_follow(self._h, status.ctypes.data_as(ip), shift.ctypes.data_as(ip),
                                                                  offset.ctypes.data_as(C.POINTER(C.c_int64)), capi.dptr(origin)))
        return status[:n.value], shift[:n.value], offset[:n.value], origin[:n.value]

    def resident_plan_goals(self, instances, goals_xy, lethal, max_sweeps=None):
        """resident_plan with world goals goals_xy [n][2] (metres): the device turns each into a cell of the instance's map as
        rolled (goal_cells' arithmetic, clamped to the map) -- for a caller whose maps follow their robots and who therefore
        cannot name a goal cell.  MPPIError (capi.ERR_STATE) while following is not set: goal_cells and resident_plan serve there."""
        inst = np.ascontiguousarray(np.atleast_1d(instances), dtype=np.int32)
        goals = capi.as_f64(np.asarray(goals_xy, dtype=np.float64).reshape(-1, 2))
        if len(goals) != len(inst):
            raise ValueError("resident_plan_goals: expected %d goals, got %d" % (len(inst), len(goals)))
        if max_sweeps is None:
            max_sweeps = self._default_sweeps(inst)
        self._check(self.lib.ccv_mppi_batch_resident_plan_goals_enqueue(self._h, len(inst), inst.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(goals),
                                                                         float(lethal), int(max_sweeps)))

    # ---- fleet term: the robots of the batch keep clear of each other (ccv_mppi_batch_resident_set_fleet) ----
    def resident_set_fleet(self, radius, range=0.0, max_neighbours=0, weight=0.0):
        """radius: one value or [B], or None (with max_neighbours = 0): the term off.  Every resident tick then appends to
        instance y's discs up to max_neighbours discs (q_j, radius[y] + radius[j]) for the nearest other robots within `range`
        of its pose at the start of the tick; weight (one value or [B]) becomes the instances' obstacle weight.  Flushes a
        pending resident update; iterate() / iterate_enqueue() are refused while the term is on."""
        reach = float(range)   # (the keyword is the C ABI's name and shadows the builtin here: use `reach` below)
        if radius is None:
            self._check(self.lib.ccv_mppi_batch_resident_set_fleet(self._h, None, reach, int(max_neighbours), None))
            return
        r = capi.as_f64(np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.B,)))
        w = capi.as_f64(np.broadcast_to(np.asarray(weight, dtype=np.float64), (self.B,)))
        self._check(self.lib.ccv_mppi_batch_resident_set_fleet(self._h, capi.dptr(r), reach, int(max_neighbours), capi.dptr(w)))

    def resident_get_fleet(self):
        """(radius [B], range, max_neighbours) as the library holds them; zeros while the term is off."""
        r = np.zeros(self.B)
        rng, m = C.c_double(), C.c_int32()
        self._check(self.lib.ccv_mppi_batch_resident_get_fleet(self._h, capi.dptr(r), C.byref(rng), C.byref(m)))
        return r, rng.value, m.value

    def resident_read_fleet(self):
        """(n_static [B], n_total [B], xyr [B][capi.MAX_OBSTACLES][3]): the disc lists the last tick's rollout was charged
        with, the static discs first, rows past n_total zero; synchronises."""
        ns, nt = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        xyr = np.zeros((self.B, capi.MAX_OBSTACLES, 3))
        self._check(self.lib.ccv_mppi_batch_resident_read_fleet(self._h, ns.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                nt.ctypes.data_as(C.POINTER(C.c_int32)), capi.dptr(xyr)))
        return ns, nt, xyr

    def resident_set_fleet_prediction(self, on=True):
        """on: every neighbour's disc moves over the horizon with the velocity that robot had over the last resident tick (its
        displacement times 1 / dt, formed on the device); off: the snapshot discs of resident_set_fleet and their bits.  Needs
        the fleet term; flushes a pending resident update."""
        self._check(self.lib.ccv_mppi_batch_set_fleet_prediction(self._h, 1 if on else 0))

    def resident_get_fleet_prediction(self):
        return bool(self.lib.ccv_mppi_batch_get_fleet_prediction(self._h))

    def resident_read_fleet_velocities(self):
        """vxy [B][capi.MAX_OBSTACLES][2]: the velocity rows the last tick's rollout was charged with, beside the disc rows of
        resident_read_fleet (rows past n_total zero); synchronises."""
        vxy = np.zeros((self.B, capi.MAX_OBSTACLES, 2))
        self._check(self.lib.ccv_mppi_batch_read_fleet_velocities(self._h, capi.dptr(vxy)))
        return vxy

    # ---- measurement ----
    def timing_enable(self, on=True, every=1):
        self._check(self.lib.ccv_mppi_batch_timing_enable(self._h, (max(1, int(every)) if on else 0)))

    def timing_read(self, reset=True):
        a, b, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self.lib.ccv_mppi_batch_timing_read(self._h, C.byref(a), C.byref(b), C.byref(n), 1 if reset else 0))
        return a.value, b.value, n.value

"""What the batch tests (tests/test_gpu_batch*.py, the batch horizon sweep and their CPU companions) share before any term is
switched on: the model makers, the cross-kernel tolerances, the kernel-flag sets, the kernel-family rule, per-instance
parameters and inputs, the paths and start poses of the resident loop, the seed of instance b, and the snapshot of everything
an iteration leaves.

Nothing here needs a GPU to import; cus() and snapshot() need one to run.  tests/test_gpu_batch_params.py checks varied,
instance_inputs, families and start_poses against single handles and the oracle, tests/test_tests_layout.py pins instance_seed
against the two spellings it replaced.
"""
import numpy as np

import ccv_mppi_path_tracker_amd as amd
import helpers
from ccv_mppi_path_tracker_amd import capi, configs
from oracle import oracle_lib as O

TOL_U = 1e-5      # as test_gpu_batch.py
TOL_COST = 1e-9
MODEL_DEFAULTS = {"diff_drive": configs.diff_drive_defaults, "steering_diff_drive": configs.steering_defaults,
                  "full_body": configs.full_body_defaults}
FAMILY_CODE = {"r4": capi.BATCH_KERNEL_FOUR_WAVE, "solo": capi.BATCH_KERNEL_ONE_WAVE}
PATHS = {}

# what last_kernel() reports beside the family: a term switches on the forms of the terms before it
SHIFT = capi.BATCH_KERNEL_SHIFT
SV = capi.BATCH_KERNEL_SHIFT | capi.BATCH_KERNEL_VARIED
OV = capi.BATCH_KERNEL_OBST | capi.BATCH_KERNEL_VARIED
MOV = capi.BATCH_KERNEL_MOVING | OV
GRID = capi.BATCH_KERNEL_GRID | MOV


def instance_seed(b, salt=0):
    """The seed of instance b: (b + 1) times the 64-bit golden-ratio constant, plus salt, modulo 2^64"""
    return (0x9E3779B97F4A7C15 * (b + 1) + salt) & 0xFFFFFFFFFFFFFFFF


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def families(model, K, B):
    """(single handle's kernel family, batch's) by the selection rule of ccv_mppi_create / ccv_mppi_batch_create"""
    ncu, nblk = cus(), -(-K // 64)    # (ncu: the local was called cus while the function was _cus)
    if model == "full_body":
        single = "r4" if nblk <= ncu else ("pc" if nblk <= 4 * ncu else "solo")
        return single, ("r4" if B * nblk <= ncu else "solo")
    return ("r4" if nblk <= 5 * ncu else "solo"), ("r4" if B * nblk <= 5 * ncu else "solo")


def varied(p, B, salt=0):
    """B parameter sets that differ from each other (and from p) in every per-instance field"""
    out = []
    for b in range(B):
        k = b + salt
        out.append(p.with_(control_noise=p.control_noise * (0.6 + 0.15 * (k % 5)), lam=p.lam * (0.5 + 0.3 * (k % 4)),
                           v_ref=p.v_ref * (0.7 + 0.1 * (k % 6)),
                           u_min=tuple(x * (1.0 + 0.05 * (k % 4)) for x in p.u_min),
                           u_max=tuple(x * (0.9 + 0.1 * (k % 3)) for x in p.u_max),
                           path_weight=p.path_weight * (1.0 + 0.5 * (k % 3)), v_weight=p.v_weight * (0.5 + 0.25 * (k % 5)),
                           zmp_weight=p.zmp_weight * (0.2 + 0.4 * (k % 3)),
                           roll_v_weight=p.roll_v_weight * (0.3 + 0.35 * (k % 4)),
                           back_weight=p.back_weight * (1.0 + (k % 3)), yaw_weight=p.yaw_weight * (0.4 + 0.3 * (k % 5))))
    return out


def instance_inputs(p, B, salt=0):
    """Distinct inputs per instance: poses along the sinusoid (even b) and dkan (odd b) paths, dt, seeds, warm starts."""
    paths = [helpers.oracle_path("sinusoid"), helpers.oracle_path("dkan")]
    nx = 5 if p.model == "full_body" else 3
    x0, xr, yr = np.zeros((B, nx)), np.zeros((B, p.horizon)), np.zeros((B, p.horizon))
    dt, yaw0 = np.zeros(B), np.zeros(B)
    seeds = np.zeros(B, dtype=np.uint64)
    rng = np.random.default_rng(4321 + salt)
    for b in range(B):
        px, py = paths[b % 2]
        i = (37 * b + 11 * salt + 5) % (len(px) // 2)
        x0[b, 0] = px[i]
        x0[b, 1] = py[i] + 0.05 * ((b % 5) - 2)
        x0[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        if nx == 5:
            x0[b, 3], x0[b, 4] = 0.02 * ((b % 3) - 1), -0.01 * (b % 2)
        dt[b] = p.dt * (1.0 + 0.05 * (b % 4))
        _, xr[b], yr[b], yaw = O.calc_ref_path(px, py, x0[b, 0], x0[b, 1], p.v_ref, dt[b], p.resolution, p.horizon)
        yaw0[b] = yaw[0]
        seeds[b] = instance_seed(b, salt)
    lo, hi = np.array(p.u_min), np.array(p.u_max)
    nom = np.clip(0.3 * (hi - lo) / 2 * rng.standard_normal((B, p.horizon - 1, p.udim)) + (hi + lo) / 2, lo, hi)
    return x0, dt, xr, yr, yaw0, seeds, nom


def close_all(*hs):
    for h in hs:
        if isinstance(h, list):
            close_all(*h)
        else:
            h.close()


def stats_tuple(s):
    return (s.sum_w, s.min_cost, s.max_cost, s.n_zero_weight, s.nonfinite)


# ---- the device-resident loop ----------------------------------------------------------------------------------------

def path_of(b):
    kind = "sinusoid" if b % 2 == 0 else "dkan"
    if kind not in PATHS:
        PATHS[kind] = amd.make_path(kind)
    return PATHS[kind]


def start_poses(p, B):
    s = np.zeros((B, p.nstate))
    seeds = np.zeros(B, dtype=np.uint64)
    for b in range(B):
        px, py = path_of(b)
        i = (37 * b + 5) % (len(px) // 2)
        s[b, 0], s[b, 1] = px[i], py[i] + 0.05 * ((b % 5) - 2)
        s[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        seeds[b] = instance_seed(b)
    return s, seeds


# ---- everything an iteration leaves ---------------------------------------------------------------------------------------

def snapshot(bat, u, st, states=True):
    B = bat.B
    return [dict(u=u[b].copy(), st=stats_tuple(st[b]), c=bat.read_costs(b), w=bat.read_weights(b),
                 xy=bat.read_candidates(b) if states else None) for b in range(B)]


def same_bits(a, b, states=True):
    keys = ("u", "c", "w") + (("xy",) if states else ())
    return a["st"] == b["st"] and all(a[k].tobytes() == b[k].tobytes() for k in keys)

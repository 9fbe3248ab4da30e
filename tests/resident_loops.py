"""The closed loop with its prologue on the host -- window, iterate, plant -- for one handle (host_loop) and for a batch
(host_batch_loop): the checker that the device-resident loops are held against bit for bit.  Beside them the resident batch
made ready to step, and the start state on a path's first point.

The host prologue itself (calc_ref_path, plant_step) is checked against the oracle in tests/test_host_prologue.py.  Used by
tests/test_gpu_resident.py, tests/test_gpu_batch_resident.py, tests/test_gpu_heading.py, tests/test_gpu_prologue_sweep.py,
tests/test_gpu_parity.py and tools/fuzz_kernels.py.  Needs no GPU to import.
"""
import numpy as np

import ccv_mppi_path_tracker_amd as amd
from batch_support import path_of
from ccv_mppi_path_tracker_amd import BatchController
from ccv_mppi_path_tracker_amd.controller import MPPIController


def start_state(p, path, lateral=0.0):
    s = np.zeros(p.nstate)
    s[0], s[1] = path[0][0], path[1][0] + lateral
    return s


def host_loop(p, px, py, s0, ticks, seed, num_samples):
    """The same closed loop with the prologue on the host: window -> iterate -> plant."""
    g = MPPIController(p, num_samples=num_samples)
    s = s0.copy()
    poses, wins, us = [], [], []
    u = None
    for it in range(ticks):
        if it > 0:
            s = amd.plant_step(p.model, s, u[0], p.dt)
        idx, xr, yr, yaw = amd.calc_ref_path(px, py, s[0], s[1], p.v_ref, p.dt, p.resolution, p.horizon)
        u = g.iterate(s, p.dt, xr, yr, yaw[0], seed, it, want_stats=False)
        poses.append(s.copy())
        wins.append((idx, xr.copy(), yr.copy(), yaw[0]))
        us.append(u.copy())
    return poses, wins, us


def host_batch_loop(p, B, K, s0, seeds, ticks, paths=None):
    """The same closed loop with the prologue on the host: per instance plant + window, then BatchController.iterate."""
    paths = paths or [path_of(b) for b in range(B)]
    bat = BatchController(p, B, num_samples=K)
    s = s0.copy()
    out, u = [], None
    for it in range(ticks):
        if it > 0:
            s = np.array([amd.plant_step(p.model, s[b], u[b][0], p.dt) for b in range(B)])
        idx, xr, yr, yaw0 = np.zeros(B, dtype=np.int64), np.zeros((B, p.horizon)), np.zeros((B, p.horizon)), np.zeros(B)
        for b in range(B):
            idx[b], xr[b], yr[b], yaw = amd.calc_ref_path(paths[b][0], paths[b][1], s[b, 0], s[b, 1], p.v_ref, p.dt,
                                                          p.resolution, p.horizon)
            yaw0[b] = yaw[0]
        u = bat.iterate(s, p.dt, xr, yr, yaw0, seeds, it, want_stats=False)
        out.append((s.copy(), idx, xr, yr, yaw0, u.copy()))
    bat.close()
    return out


def resident_batch(p, B, K, s0, seeds, paths=None):
    bat = BatchController(p, B, num_samples=K)
    bat.resident_set_paths(paths or [path_of(b) for b in range(B)])
    bat.resident_set_poses(s0, seeds)
    return bat

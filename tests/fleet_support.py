"""The fleets of the batch tests (DESIGN.md sections 10f and 10g): robots of one resident batch along the sinusoid path, static
discs far from any rollout that only fill rows, a handle made with its terms in one call, everything a tick leaves as bytes,
and the parameters of the two behaviour tests -- two robots head on, two robots crossing.

tests/test_gpu_batch_fleet.py holds handles made this way against a twin fed through set_obstacles, bit for bit;
tests/test_fleet_head_on_cpu.py and tests/test_fleet_crossing_cpu.py pin HEAD_ON and CROSSING on the CPU restatements of the
closed loop (tools/fleet_head_on_cpu.py, tools/fleet_crossing_cpu.py).  Needs no GPU to import; make() needs one to run.
"""
import os
import sys

import numpy as np

import batch_support as BS
from ccv_mppi_path_tracker_amd import BatchController

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fleet_crossing_cpu as FC  # noqa: E402

FAR = 40.0   # static discs this far from the paths never touch a rollout: they fill rows


def params(model="diff_drive", K=128, H=15):
    return BS.MODEL_DEFAULTS[model](K, H)


def fleet_start(p, B, first=5, step=3):
    """B robots on the sinusoid path, `step` path points (0.1 m each) apart, with small lateral offsets"""
    px, py = BS.path_of(0)
    s = np.zeros((B, p.nstate))
    seeds = np.zeros(B, dtype=np.uint64)
    for b in range(B):
        i = first + step * b
        s[b, 0], s[b, 1] = px[i], py[i] + 0.05 * ((b % 5) - 2)
        s[b, 2] = np.arctan2(py[i + 1] - py[i], px[i + 1] - px[i]) + 0.1 * ((b % 3) - 1)
        seeds[b] = BS.instance_seed(b)
    return s, seeds, [BS.path_of(0)] * B


def far_discs(n, salt=0):
    a = 0.7 * np.arange(n) + salt
    return np.stack([FAR * np.cos(a) + 5.0, FAR * np.sin(a), 0.5 + 0.01 * np.arange(n)], axis=1).reshape(-1, 3)


def bits(bat):
    """everything a tick leaves, as bytes per field"""
    st, idx, xr, yr, _, steps = bat.resident_read()
    return dict(u=bat.get_nominal().tobytes(), st=st.tobytes(), idx=idx.tobytes(), xr=xr.tobytes(), yr=yr.tobytes(), steps=steps,
                c=b"".join(bat.read_costs(b).tobytes() for b in range(bat.B)))


def robot_bits(bat, b):
    st, idx = bat.resident_read()[:2]
    return (bat.get_nominal()[b].tobytes(), st[b].tobytes(), int(idx[b]), bat.read_costs(b).tobytes())


def make(p, B, shift, static, weight, paths, s0, seeds, fleet=None, timed=False):
    bat = BatchController(p, B, min_shift=shift)
    if static is not None:
        bat.set_obstacles(static, weight)
    bat.resident_set_paths(paths)
    bat.resident_set_poses(s0, seeds)
    if fleet is not None:
        bat.resident_set_fleet(*fleet)
    if timed:
        bat.timing_enable(True)
    return bat


# ---- behaviour ------------------------------------------------------------------------------------------------------------
_X = 0.1 * np.arange(61)
# chosen on the CPU restatement of the closed loop (tools/fleet_head_on_cpu.py; tests/test_fleet_head_on_cpu.py)
HEAD_ON = dict(paths=[(_X, np.zeros(61)), (_X[::-1].copy(), np.zeros(61))], s0=np.array([[1.5, 0.0, 0.0], [4.5, 0.0, np.pi]]),
               seeds=np.array([11, 12], dtype=np.uint64), ticks=90, radius=0.3, range=3.0, weight=200.0)

# chosen on the CPU restatement of the closed loop (tools/fleet_crossing_cpu.py; tests/test_fleet_crossing_cpu.py)
CROSSING = dict(paths=FC.PATHS, s0=FC.S0, seeds=np.array([11, 12], dtype=np.uint64), ticks=60, radius=0.1, range=3.0, weight=100.0,
                margin=0.08)

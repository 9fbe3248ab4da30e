"""The horizon arithmetic of the rollout kernels, restated in plain Python, and the horizons the sweep tests run
(tests/test_gpu_horizon_sweep.py, tests/test_gpu_horizon_sweep_batch.py; tests/test_horizon_cases_cpu.py proves what they reach).

Every rollout kernel cuts the horizon into blocks of kTU = 8 steps and handles the last block by H:

  nblocks    (H + kTU - 1) / kTU: the first line of every kernel's time loop (mppi_rollout_r4.h, _r3.h, _pc.h, _solo.h).
  nctl_last  min(kTU, H - 1 - kTU b) at the last block b = nblocks - 1: the control steps of that block, read by the dynamics
             wave of each kernel (`nctl`) to choose the full batch (8), the masked PARTIAL batch of pc_produce_batched
             (kPartialMin .. 7) or the step-by-step pc_produce (0 .. 3).
  nv_last    min(kTU, nstates - kTU b) at the last block, nstates = H (diff drive, steering) or H - 2 (full body): the states
             of that block that reach the path cost, read by the distance wave to pick one of pc_consume<1..8>; it can be <= 0
             for full body, and then the wave takes nothing of the block (`taken` false).
  tail       (H - 1) % kTU >= kPartialMin: launch_rollout() in mppi_launch.hip, which picks the four-wave kernel's TAIL
             instantiation (and the batch units') by it.
  nfull      the blocks whose normals the four-wave kernel's noise wave makes: (H - 1 + kTU - kPartialMin) / kTU with TAIL,
             (H - 1) / kTU without (mppi_rollout_r4.h, fused iteration).
  prune      H > 16: select_kernels() in ccv_mppi_capi.hip switches the exact window pruning of the distance loop on there.
"""
K_TU = 8
K_PARTIAL_MIN = 4

MODELS = ("diff_drive", "steering_diff_drive", "full_body")
SINGLE_H = tuple(range(3, 27))    # one, two, three and four blocks, every residue in each
BATCH_H = tuple(range(5, 27))     # (below 5 full body has nstates <= 2: no disc can be placed on its rollouts)


def nstates(model, H):
    return H - 2 if model == "full_body" else H


def block_shape(model, H):
    """(nblocks, nctl_last, nv_last, tail, nfull, prune) of horizon H"""
    nblocks = (H + K_TU - 1) // K_TU
    last = nblocks - 1
    nctl_last = min(K_TU, H - 1 - K_TU * last)
    nv_last = min(K_TU, nstates(model, H) - K_TU * last)
    tail = (H - 1) % K_TU >= K_PARTIAL_MIN
    nfull = (H - 1 + K_TU - K_PARTIAL_MIN) // K_TU if tail else (H - 1) // K_TU
    prune = H > 16
    return nblocks, nctl_last, nv_last, tail, nfull, prune


def consumer_widths(model, H):
    """every nv > 0 the distance wave dispatches pc_consume<nv> with over the blocks of horizon H"""
    nblocks = block_shape(model, H)[0]
    return [nv for nv in (min(K_TU, nstates(model, H) - K_TU * b) for b in range(nblocks)) if nv > 0]


def producer_steps(H):
    """nctl of every block of horizon H"""
    nblocks = (H + K_TU - 1) // K_TU
    return [min(K_TU, H - 1 - K_TU * b) for b in range(nblocks)]


# The one case of the batch sweep whose inputs are not BS.instance_inputs(p, 5) with salt 0: steering H = 5 with salt 0 gives a
# moving-disc instance every sample of which carries a penalty (share 1.00; the condition is 10 % .. 90 %).
BATCH_SALT = {("steering_diff_drive", 5): 1}


def batch_salt(model, H):
    return BATCH_SALT.get((model, H), 0)

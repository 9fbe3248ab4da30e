// translation unit: the batch handles' kernels with block-relative shifted weights (ccv_mppi_batch_set_min_shift; SHIFT,
// pc_shifted_weight in mppi_rollout_pc.h) -- the four-wave and one-wave rollout kernels of every model, on top of the
// per-instance-parameter forms only (a handle without ccv_mppi_batch_set_params has B copies of its configuration in the
// table).  The plain family keeps k_batch_varied.hip's kernel: its weights are re-formed with the exact instance minimum
// (k_min_cost_batch, k_reweight_batch in k_update.hip).  A unit of its own, like k_batch_varied.hip.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_shift_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.family == KernelFamily::OneWave) {
        launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, true, true, true>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
    } else {
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, true, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, true, true, true>, grid, block, at, A, W);
    }
}

// (p.family: FourWave or OneWave)
void launch_batch_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_shift_model<CCV_MPPI_DIFF_DRIVE, true>(p, tail, at, A, W);
        else launch_shift_model<CCV_MPPI_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_shift_model<CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else {
        launch_shift_model<CCV_MPPI_FULL_BODY, false>(p, tail, at, A, W);
    }
}

}  // namespace ccv

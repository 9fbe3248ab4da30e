// translation unit: the four-wave rollout kernel (mppi_rollout_r4.h), diff drive and steering, single and batch handles (full
// body: k_r4_fb.hip, its batch form k_batch.hip)
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"

namespace ccv {

// single handle: every mode; batch (p.batch instances): the fused iteration
template <int MODEL>
static void launch_r4_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
    if (p.batch) {
        if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
            if (p.wide) {
                if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, true, BatchForm::Batch>, grid, block, at, A, W);
                else launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, false, BatchForm::Batch>, grid, block, at, A, W);
                return;
            }
        }
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true, BatchForm::Batch>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, false, BatchForm::Batch>, grid, block, at, A, W);
        return;
    }
    if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
        if (p.mode == MODE_FUSED && p.wide) {
            if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, true>, grid, block, at, A, W);
            else launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, false>, grid, block, at, A, W);
            return;
        }
    }
    if (p.mode == MODE_FUSED && tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true>, grid, block, at, A, W);
    else if (p.mode == MODE_FUSED) launch_at(k_rollout_r4<MODEL, MODE_FUSED>, grid, block, at, A, W);
    else if (p.mode == MODE_ROLLOUT) launch_at(k_rollout_r4<MODEL, MODE_ROLLOUT>, grid, block, at, A, W);
    else launch_at(k_rollout_r4<MODEL, MODE_COST>, grid, block, at, A, W);
}

void launch_r4(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) launch_r4_model<CCV_MPPI_DIFF_DRIVE>(p, tail, at, A, W);
    else launch_r4_model<CCV_MPPI_STEERING_DIFF_DRIVE>(p, tail, at, A, W);
}

}  // namespace ccv

// translation unit: the one-wave rollout kernel (mppi_rollout_solo.h), diff drive and steering; full body: k_solo_fb.hip
#include "mppi_launch.h"
#include "mppi_rollout_solo.h"

namespace ccv {

void launch_solo(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, 0), block(kPcSamples);
    if (p.model != CCV_MPPI_DIFF_DRIVE) launch_at(k_rollout_solo<CCV_MPPI_STEERING_DIFF_DRIVE, MODE_FUSED>, grid, block, at, A, W);
    else if (p.wide) launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED, true>, grid, block, at, A, W);
    else launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED>, grid, block, at, A, W);
}

}  // namespace ccv

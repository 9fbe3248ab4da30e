// translation unit: the two-wave rollout kernel (mppi_rollout_pc.h), diff drive and steering (experiments, CCV_MPPI_KERNEL=pc);
// full body: k_pc_fb.hip
#include "mppi_launch.h"
#include "mppi_rollout_pc.h"

namespace ccv {

template <int MODEL>
static void launch_pc_model(int mode, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, 0), block(kPcWaves * 64);
    if (mode == MODE_FUSED) launch_at(k_rollout_pc<MODEL, MODE_FUSED>, grid, block, at, A, W);
    else if (mode == MODE_ROLLOUT) launch_at(k_rollout_pc<MODEL, MODE_ROLLOUT>, grid, block, at, A, W);
    else launch_at(k_rollout_pc<MODEL, MODE_COST>, grid, block, at, A, W);
}

void launch_pc(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) launch_pc_model<CCV_MPPI_DIFF_DRIVE>(p.mode, at, A, W);
    else launch_pc_model<CCV_MPPI_STEERING_DIFF_DRIVE>(p.mode, at, A, W);
}

}  // namespace ccv

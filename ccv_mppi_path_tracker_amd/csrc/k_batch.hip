// translation unit: the batch handles' forms of the one-wave kernel (all models) and of the full-body four-wave kernel (their
// diff-drive / steering four-wave and plain forms live beside the single handle's, k_r4.hip / k_plain.hip).  A unit of its own:
// next to the single handle's instantiations in k_solo*.hip / k_r4_fb.hip they changed the code hipcc generated for those.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_solo_batch(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, true>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
}

void launch_batch(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.family == KernelFamily::FourWave) {   // full body
        constexpr int MODEL = CCV_MPPI_FULL_BODY;
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, false, true>, grid, block, at, A, W);
    } else if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_solo_batch<CCV_MPPI_DIFF_DRIVE, true>(p, at, A, W);
        else launch_solo_batch<CCV_MPPI_DIFF_DRIVE, false>(p, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_solo_batch<CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, at, A, W);
    } else {
        launch_solo_batch<CCV_MPPI_FULL_BODY, false>(p, at, A, W);
    }
}

}  // namespace ccv

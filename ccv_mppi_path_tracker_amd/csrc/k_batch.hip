// translation unit: the batch handles' forms of the one-wave kernel (all models) and of the full-body four-wave kernel (their
// diff-drive / steering four-wave and plain forms live beside the single handle's, k_r4.hip / k_plain.hip).  A unit of its own:
// next to the single handle's instantiations in k_solo*.hip / k_r4_fb.hip they changed the code hipcc generated for those.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

void launch_rollout_solo_batch(int model, bool wide, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, batch), block(kPcSamples);
    if (model == CCV_MPPI_DIFF_DRIVE) {
        if (wide) launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED, false, true>, grid, block, at, A, W);
    } else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_at(k_rollout_solo<CCV_MPPI_STEERING_DIFF_DRIVE, MODE_FUSED, false, true>, grid, block, at, A, W);
    } else {
        launch_at(k_rollout_solo<CCV_MPPI_FULL_BODY, MODE_FUSED, false, true>, grid, block, at, A, W);
    }
}

void launch_rollout_r4_fb_batch(int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    constexpr int MODEL = CCV_MPPI_FULL_BODY;
    const dim3 grid = blocks_of_64(A, batch), block(kR4Waves * 64);
    if ((A.H - 1) % kTU >= kPartialMin) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true, true>, grid, block, at, A, W);
    else launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, false, true>, grid, block, at, A, W);
}

}  // namespace ccv

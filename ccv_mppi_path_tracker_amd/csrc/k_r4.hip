// translation unit: the four-wave rollout kernel (mppi_rollout_r4.h), diff drive and steering, single and batch handles (full
// body: k_r4_fb.hip, its batch form k_batch.hip)
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"

namespace ccv {

template <int MODEL>
static void launch_r4_model(int mode, bool wide, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A), block(kR4Waves * 64);
    // the horizon's tail: kPartialMin .. 7 control steps in the last block -> the instantiation with the masked batch producer
    const bool tail = (A.H - 1) % kTU >= kPartialMin;
    if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
        if (mode == MODE_FUSED && wide) {
            if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, true>, grid, block, at, A, W);
            else launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, false>, grid, block, at, A, W);
            return;
        }
    }
    if (mode == MODE_FUSED && tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true>, grid, block, at, A, W);
    else if (mode == MODE_FUSED) launch_at(k_rollout_r4<MODEL, MODE_FUSED>, grid, block, at, A, W);
    else if (mode == MODE_ROLLOUT) launch_at(k_rollout_r4<MODEL, MODE_ROLLOUT>, grid, block, at, A, W);
    else launch_at(k_rollout_r4<MODEL, MODE_COST>, grid, block, at, A, W);
}

void launch_rollout_r4_fb(int mode, const LaunchAt& at, const RolloutArgs& A, const Window& W);   // k_r4_fb.hip
void launch_rollout_r4_fb_batch(int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W);   // k_batch.hip

template <int MODEL>
static void launch_r4_batch_model(bool wide, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, batch), block(kR4Waves * 64);
    const bool tail = (A.H - 1) % kTU >= kPartialMin;
    if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
        if (wide) {
            if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, true, true>, grid, block, at, A, W);
            else launch_at(k_rollout_r4<MODEL, MODE_FUSED, true, false, true>, grid, block, at, A, W);
            return;
        }
    }
    if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, true, true>, grid, block, at, A, W);
    else launch_at(k_rollout_r4<MODEL, MODE_FUSED, false, false, true>, grid, block, at, A, W);
}

void launch_rollout_r4_batch(int model, bool wide, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (model == CCV_MPPI_DIFF_DRIVE) launch_r4_batch_model<CCV_MPPI_DIFF_DRIVE>(wide, batch, at, A, W);
    else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) launch_r4_batch_model<CCV_MPPI_STEERING_DIFF_DRIVE>(false, batch, at, A, W);
    else launch_rollout_r4_fb_batch(batch, at, A, W);
}

void launch_rollout_r4(int model, int mode, bool wide, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (model == CCV_MPPI_DIFF_DRIVE) launch_r4_model<CCV_MPPI_DIFF_DRIVE>(mode, wide, at, A, W);
    else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) launch_r4_model<CCV_MPPI_STEERING_DIFF_DRIVE>(mode, false, at, A, W);
    else launch_rollout_r4_fb(mode, at, A, W);
}

}  // namespace ccv

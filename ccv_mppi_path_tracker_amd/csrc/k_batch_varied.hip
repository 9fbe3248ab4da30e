// translation unit: the batch handles' kernels with per-instance parameters (ccv_mppi_batch_set_params; VARIED, batch_view in
// mppi_kernels.h) -- the four-wave, one-wave and plain rollout kernels of every model.  A unit of its own, like k_batch.hip:
// the instantiations beside the existing ones could change the code hipcc generates for those.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_r4_varied_model(int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, batch), block(kR4Waves * 64);
    if ((A.H - 1) % kTU >= kPartialMin) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, true, true>, grid, block, at, A, W);
    else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, true, true>, grid, block, at, A, W);
}

void launch_rollout_r4_batch_varied(int model, bool wide, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (model == CCV_MPPI_DIFF_DRIVE) {
        if (wide) launch_r4_varied_model<CCV_MPPI_DIFF_DRIVE, true>(batch, at, A, W);
        else launch_r4_varied_model<CCV_MPPI_DIFF_DRIVE, false>(batch, at, A, W);
    } else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_r4_varied_model<CCV_MPPI_STEERING_DIFF_DRIVE, false>(batch, at, A, W);
    } else {
        launch_r4_varied_model<CCV_MPPI_FULL_BODY, false>(batch, at, A, W);
    }
}

void launch_rollout_solo_batch_varied(int model, bool wide, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid = blocks_of_64(A, batch), block(kPcSamples);
    if (model == CCV_MPPI_DIFF_DRIVE) {
        if (wide) launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED, true, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_solo<CCV_MPPI_DIFF_DRIVE, MODE_FUSED, false, true, true>, grid, block, at, A, W);
    } else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_at(k_rollout_solo<CCV_MPPI_STEERING_DIFF_DRIVE, MODE_FUSED, false, true, true>, grid, block, at, A, W);
    } else {
        launch_at(k_rollout_solo<CCV_MPPI_FULL_BODY, MODE_FUSED, false, true, true>, grid, block, at, A, W);
    }
}

// grid (workgroups per instance, instances), as launch_rollout_plain_batch
void launch_rollout_plain_batch_varied(int model, int batch, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const dim3 grid((unsigned)((A.K + kBlock - 1) / kBlock), (unsigned)batch), block(kBlock);
    if (model == CCV_MPPI_DIFF_DRIVE) launch_at(k_rollout_cost<CCV_MPPI_DIFF_DRIVE, SRC_PHILOX, true, true, true>, grid, block, at, A, W);
    else if (model == CCV_MPPI_STEERING_DIFF_DRIVE) launch_at(k_rollout_cost<CCV_MPPI_STEERING_DIFF_DRIVE, SRC_PHILOX, true, true, true>, grid, block, at, A, W);
    else launch_at(k_rollout_cost<CCV_MPPI_FULL_BODY, SRC_PHILOX, true, true, true>, grid, block, at, A, W);
}

}  // namespace ccv

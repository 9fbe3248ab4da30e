// translation unit: the batch handles' kernels with per-instance parameters (ccv_mppi_batch_set_params; VARIED, batch_view in
// mppi_kernels.h) -- the four-wave, one-wave and plain rollout kernels of every model.  A unit of its own, like k_batch.hip:
// the instantiations beside the existing ones could change the code hipcc generates for those.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_varied_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.family == KernelFamily::Plain) {
        launch_at(k_rollout_cost<MODEL, SRC_PHILOX, true, true, true>, blocks_plain(A, p.batch), dim3(kBlock), at, A, W);
    } else if (p.family == KernelFamily::OneWave) {
        launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, true, true>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
    } else {
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, true, true>, grid, block, at, A, W);
    }
}

void launch_batch_varied(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_varied_model<CCV_MPPI_DIFF_DRIVE, true>(p, tail, at, A, W);
        else launch_varied_model<CCV_MPPI_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_varied_model<CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else {
        launch_varied_model<CCV_MPPI_FULL_BODY, false>(p, tail, at, A, W);
    }
}

}  // namespace ccv

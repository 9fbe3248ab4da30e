// translation unit: the batch handles' kernels with a per-instance occupancy GRID AND block-relative shifted weights (GRID on
// MOVING on OBST on SHIFT on VARIED) -- the four-wave and one-wave rollout kernels of every model, the twelve forms of
// k_batch_grid_shift.hip.  The plain family keeps k_batch_grid.hip's kernel (its weights are re-formed with the exact instance
// minimum).  A unit of its own.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_grid_shift_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.family == KernelFamily::OneWave) {
        // (full body: no one-wave grid form -- make_plan sends those plans to the four-wave kernel)
        if constexpr (MODEL != CCV_MPPI_FULL_BODY) {
            launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, true, true, true, true, true, true>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
        }
    } else {
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, true, true, true, true, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, true, true, true, true, true, true>, grid, block, at, A, W);
    }
}

// (p.family: FourWave or OneWave)
void launch_batch_grid_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_grid_shift_model<CCV_MPPI_DIFF_DRIVE, true>(p, tail, at, A, W);
        else launch_grid_shift_model<CCV_MPPI_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_grid_shift_model<CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else {
        launch_grid_shift_model<CCV_MPPI_FULL_BODY, false>(p, tail, at, A, W);
    }
}

}  // namespace ccv

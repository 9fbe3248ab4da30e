// translation unit: the batch handles' kernels with a per-instance occupancy GRID (ccv_mppi_batch_set_grids; GRID on MOVING,
// grid_tap in mppi_kernels.h) and unshifted weights -- the four-wave, one-wave and plain rollout kernels of every model, the
// forms of k_batch_grid.hip.  The shifted-weight forms: k_batch_grid_shift.hip.  A unit of its own.
#include "mppi_launch.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <int MODEL, bool WIDE>
static void launch_grid_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.family == KernelFamily::Plain) {
        launch_at(k_rollout_cost<MODEL, SRC_PHILOX, true, true, true, true, true, true>, blocks_plain(A, p.batch), dim3(kBlock), at, A, W);
    } else if (p.family == KernelFamily::OneWave) {
        // (full body: no one-wave grid form -- make_plan sends those plans to the four-wave kernel)
        if constexpr (MODEL != CCV_MPPI_FULL_BODY) {
            launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, true, true, false, true, true, true>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
        }
    } else {
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, true, true, false, true, true, true>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, true, true, false, true, true, true>, grid, block, at, A, W);
    }
}

void launch_batch_grid_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);   // k_batch_grid_shift.hip

// (shifted weights: the plain family keeps this unit's kernel -- the host re-forms its weights, k_reweight_batch)
void launch_batch_grid(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.shift && p.family != KernelFamily::Plain) return launch_batch_grid_shift(p, tail, at, A, W);
    if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_grid_model<CCV_MPPI_DIFF_DRIVE, true>(p, tail, at, A, W);
        else launch_grid_model<CCV_MPPI_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_grid_model<CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else {
        launch_grid_model<CCV_MPPI_FULL_BODY, false>(p, tail, at, A, W);
    }
}

}  // namespace ccv

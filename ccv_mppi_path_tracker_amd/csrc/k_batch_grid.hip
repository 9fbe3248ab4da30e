// translation unit: the batch handles' kernels with a per-instance occupancy GRID (ccv_mppi_batch_set_grids; GRID on MOVING,
// grid_tap in mppi_cost_terms.h) and unshifted weights -- the four-wave, one-wave and plain rollout kernels of every model, the
// forms of k_batch_moving.hip but the one-wave full-body kernel, which has no grid form.  The shifted-weight forms:
// k_batch_grid_shift.hip.  A unit of its own.
#include "k_batch_form.h"

namespace ccv {

void launch_batch_grid(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Grid, false>(p, tail, at, A, W);
}

}  // namespace ccv

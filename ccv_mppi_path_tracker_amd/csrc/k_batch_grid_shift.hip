// translation unit: the batch handles' kernels with a per-instance occupancy GRID AND block-relative shifted weights (GRID on
// MOVING on OBST on SHIFT on VARIED) -- the four-wave and one-wave rollout kernels of every model, the forms of
// k_batch_moving_shift.hip but the one-wave full-body kernel.  The plain family keeps k_batch_grid.hip's kernel (its weights are
// re-formed with the exact instance minimum).  A unit of its own.
#include "k_batch_form.h"

namespace ccv {

// (p.family: FourWave or OneWave)
void launch_batch_grid_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Grid, true>(p, tail, at, A, W);
}

}  // namespace ccv

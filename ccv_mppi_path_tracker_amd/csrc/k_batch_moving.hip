// translation unit: the batch handles' kernels with per-instance MOVING disc obstacles (ccv_mppi_batch_set_obstacle_velocities;
// MOVING on OBST, obst_stage_moving / obst_term_moving in mppi_cost_terms.h) and unshifted weights -- the four-wave, one-wave and
// plain rollout kernels of every model, the forms of k_batch_obst.hip.  The shifted-weight forms: k_batch_moving_shift.hip.  A
// unit of its own.
#include "k_batch_form.h"

namespace ccv {

void launch_batch_moving(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Moving, false>(p, tail, at, A, W);
}

}  // namespace ccv

// translation unit: the batch handles' kernels with per-instance disc obstacles (ccv_mppi_batch_set_obstacles; OBST, obst_stage /
// obst_term in mppi_cost_terms.h) and unshifted weights -- the four-wave, one-wave and plain rollout kernels of every model, on top
// of the per-instance-parameter forms only (a handle without ccv_mppi_batch_set_params has B copies of its configuration in the
// table).  The shifted-weight forms: k_batch_obst_shift.hip.  A unit of its own, like k_batch_varied.hip.
#include "k_batch_form.h"

namespace ccv {

void launch_batch_obst(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Obst, false>(p, tail, at, A, W);
}

}  // namespace ccv

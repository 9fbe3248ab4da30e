// translation unit: the batch handles' kernels with block-relative shifted weights (ccv_mppi_batch_set_min_shift; SHIFT,
// pc_shifted_weight in mppi_epilogue.h) -- the four-wave and one-wave rollout kernels of every model, on top of the
// per-instance-parameter forms only (a handle without ccv_mppi_batch_set_params has B copies of its configuration in the
// table).  The plain family keeps k_batch_varied.hip's kernel: its weights are re-formed with the exact instance minimum
// (k_min_cost_batch, k_reweight_batch in k_update.hip).  A unit of its own, like k_batch_varied.hip.
#include "k_batch_form.h"

namespace ccv {

// (p.family: FourWave or OneWave)
void launch_batch_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Varied, true>(p, tail, at, A, W);
}

}  // namespace ccv

// translation unit: the batch handles' kernels with per-instance disc obstacles AND block-relative shifted weights (OBST on SHIFT
// on VARIED) -- the four-wave and one-wave rollout kernels of every model, the twelve forms of k_batch_shift.hip.  The plain
// family keeps k_batch_obst.hip's kernel (its weights are re-formed with the exact instance minimum).  A unit of its own.
#include "k_batch_form.h"

namespace ccv {

// (p.family: FourWave or OneWave)
void launch_batch_obst_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Obst, true>(p, tail, at, A, W);
}

}  // namespace ccv

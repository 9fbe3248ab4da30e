// translation unit: the batch handles' kernels with per-instance parameters (ccv_mppi_batch_set_params; VARIED, batch_view in
// mppi_kernels.h) -- the four-wave, one-wave and plain rollout kernels of every model.  A unit of its own, like k_batch.hip:
// the instantiations beside the existing ones could change the code hipcc generates for those.
#include "k_batch_form.h"

namespace ccv {

void launch_batch_varied(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Varied, false>(p, tail, at, A, W);
}

}  // namespace ccv

// translation unit: the batch handles' forms of the one-wave kernel (all models) and of the full-body four-wave kernel (their
// diff-drive / steering four-wave and plain forms live beside the single handle's, k_r4.hip / k_plain.hip).  A unit of its own:
// next to the single handle's instantiations in k_solo*.hip / k_r4_fb.hip they changed the code hipcc generated for those.
#include "k_batch_form.h"

namespace ccv {

void launch_batch(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    launch_batch_form<BatchForm::Batch, false>(p, tail, at, A, W);
}

}  // namespace ccv

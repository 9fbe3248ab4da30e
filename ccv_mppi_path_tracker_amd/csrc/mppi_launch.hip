// launch_rollout(): from a RolloutPlan to the translation unit that holds the kernel (mppi_launch.h: why the units).  Host code
// only; no kernel is instantiated here.
#include "mppi_launch.h"

namespace ccv {

// one launcher per unit.  tail: kPartialMin .. 7 control steps in the horizon's last block of kTU -> the four-wave kernel's
// instantiation with the masked batch producer
void launch_r4(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);      // k_r4.hip: dd, sd; their batch form
void launch_r4_fb(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);   // k_r4_fb.hip
void launch_r3(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);                 // k_r3.hip: dd, sd
void launch_pc(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);                 // k_pc.hip: dd, sd
void launch_pc_fb(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);              // k_pc_fb.hip
void launch_solo(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);               // k_solo.hip: dd, sd
void launch_solo_fb(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);            // k_solo_fb.hip
void launch_plain(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W);              // k_plain.hip: its batch form too
// the batch units, one per rung of BatchForm and shift (k_batch_form.h).  k_batch.hip: one-wave, fb four-wave; the unshifted units:
// all three families; the _shift units: four-, one-wave
void launch_batch(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_varied(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_obst(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_obst_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_moving(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_moving_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_grid(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_batch_grid_shift(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W);

void launch_rollout(const RolloutPlan& p, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    const bool fb = p.model == CCV_MPPI_FULL_BODY;
    const bool tail = (A.H - 1) % kTU >= kPartialMin;
    // (shifted weights: the plain family keeps the unshifted unit's kernel -- the host re-forms its weights, k_reweight_batch)
    const bool shift = p.shift && p.family != KernelFamily::Plain;
    switch (p.form) {
    case BatchForm::Grid: return shift ? launch_batch_grid_shift(p, tail, at, A, W) : launch_batch_grid(p, tail, at, A, W);
    case BatchForm::Moving: return shift ? launch_batch_moving_shift(p, tail, at, A, W) : launch_batch_moving(p, tail, at, A, W);
    case BatchForm::Obst: return shift ? launch_batch_obst_shift(p, tail, at, A, W) : launch_batch_obst(p, tail, at, A, W);
    case BatchForm::Varied: return shift ? launch_batch_shift(p, tail, at, A, W) : launch_batch_varied(p, tail, at, A, W);
    case BatchForm::Batch:   // (its diff-drive / steering four-wave and plain kernels: beside the single handle's)
        if (p.family == KernelFamily::Plain) return launch_plain(p, at, A, W);
        return p.family == KernelFamily::FourWave && !fb ? launch_r4(p, tail, at, A, W) : launch_batch(p, tail, at, A, W);
    case BatchForm::Single: break;
    }
    switch (p.family) {
    case KernelFamily::Plain: return launch_plain(p, at, A, W);
    case KernelFamily::TwoWave: return fb ? launch_pc_fb(p, at, A, W) : launch_pc(p, at, A, W);
    case KernelFamily::ThreeWave: return launch_r3(p, at, A, W);
    case KernelFamily::FourWave: return fb ? launch_r4_fb(p, tail, at, A, W) : launch_r4(p, tail, at, A, W);
    case KernelFamily::OneWave: return fb ? launch_solo_fb(p, at, A, W) : launch_solo(p, at, A, W);
    }
}

}  // namespace ccv

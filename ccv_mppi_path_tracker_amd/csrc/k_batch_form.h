// The launcher of the batch units k_batch*.hip, written once: from a plan to the kernel of one <FORM, SHIFT> (BatchForm,
// mppi_kernels.h).  Each unit includes this and names its pair in one external function, so each unit instantiates exactly its
// own kernels (mppi_launch.h: why the units).  What a pair does not build falls out below at compile time; launch_rollout()
// (mppi_launch.hip) sends no such plan here.
#pragma once
#include "mppi_launch.h"
#include "mppi_rollout_plain.h"
#include "mppi_rollout_r4.h"
#include "mppi_rollout_solo.h"

namespace ccv {

template <BatchForm FORM, bool SHIFT, int MODEL, bool WIDE>
static void launch_batch_form_model(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    constexpr bool FB = MODEL == CCV_MPPI_FULL_BODY;
    if (p.family == KernelFamily::Plain) {
        // (shifted weights: the plain family keeps the unshifted unit's kernel -- the host re-forms its weights, k_reweight_batch;
        //  Batch: k_plain.hip)
        if constexpr (!SHIFT && FORM != BatchForm::Batch) {
            launch_at(k_rollout_cost<MODEL, SRC_PHILOX, true, FORM>, blocks_plain(A, p.batch), dim3(kBlock), at, A, W);
        }
    } else if (p.family == KernelFamily::OneWave) {
        // (full body: no one-wave grid form -- make_plan sends those plans to the four-wave kernel)
        if constexpr (has_one_wave_form(MODEL, FORM)) {
            launch_at(k_rollout_solo<MODEL, MODE_FUSED, WIDE, FORM, SHIFT>, blocks_of_64(A, p.batch), dim3(kPcSamples), at, A, W);
        }
    } else if constexpr (FB || FORM != BatchForm::Batch) {   // (Batch, diff drive and steering: k_r4.hip)
        const dim3 grid = blocks_of_64(A, p.batch), block(kR4Waves * 64);
        if (tail) launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, true, FORM, SHIFT>, grid, block, at, A, W);
        else launch_at(k_rollout_r4<MODEL, MODE_FUSED, WIDE, false, FORM, SHIFT>, grid, block, at, A, W);
    }
}

template <BatchForm FORM, bool SHIFT>
static void launch_batch_form(const RolloutPlan& p, bool tail, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (p.model == CCV_MPPI_DIFF_DRIVE) {
        if (p.wide) launch_batch_form_model<FORM, SHIFT, CCV_MPPI_DIFF_DRIVE, true>(p, tail, at, A, W);
        else launch_batch_form_model<FORM, SHIFT, CCV_MPPI_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else if (p.model == CCV_MPPI_STEERING_DIFF_DRIVE) {
        launch_batch_form_model<FORM, SHIFT, CCV_MPPI_STEERING_DIFF_DRIVE, false>(p, tail, at, A, W);
    } else {
        launch_batch_form_model<FORM, SHIFT, CCV_MPPI_FULL_BODY, false>(p, tail, at, A, W);
    }
}

}  // namespace ccv

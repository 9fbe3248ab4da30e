// Launching a rollout kernel.  Which kernel a launch runs is a value, RolloutPlan; launch_rollout() (mppi_launch.hip) is a
// switch over it.  Every family is a translation unit of its own (k_r4.hip, k_r3.hip, k_pc.hip, k_r4_fb.hip, k_pc_fb.hip,
// k_solo.hip, k_solo_fb.hip, k_plain.hip), and so is every rung of the batch handles' BatchForm (mppi_kernels.h) with and without
// shifted weights (k_batch.hip; k_batch_varied.hip, k_batch_shift.hip; k_batch_obst.hip, k_batch_obst_shift.hip;
// k_batch_moving.hip, k_batch_moving_shift.hip; k_batch_grid.hip, k_batch_grid_shift.hip -- one launcher, k_batch_form.h, which
// each of them names once): hipcc spends over a minute on all instantiations in one file, the units compile side by side
// (build.py), and an instantiation placed beside others can change the code generated for those.  The C ABI picks the family at
// create (select_kernels(), ccv_mppi_capi.hip) and makes the plan of each launch from it (make_plan(), capi_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "mppi_kernels.h"

namespace ccv {

// where a rollout kernel is launched: the stream and, for a timed launch, the events attached to the dispatch itself
// (kernel begin / end timestamps: hipExtLaunchKernelGGL); null events = a plain launch
struct LaunchAt {
    hipStream_t stream;
    hipEvent_t ev_start, ev_stop;
};

// Plain: one sample per lane, OCML sincos (unbounded headings, CCV_MPPI_KERNEL=v1); TwoWave: mppi_rollout_pc.h; ThreeWave:
// mppi_rollout_r3.h (diff drive, steering); FourWave: mppi_rollout_r4.h; OneWave: mppi_rollout_solo.h (fused iteration only)
enum class KernelFamily : int { Plain, TwoWave, ThreeWave, FourWave, OneWave };

struct RolloutPlan {
    KernelFamily family;
    int model;
    int mode;          // MODE_FUSED / MODE_ROLLOUT / MODE_COST (mppi_kernels.h)
    bool wide;         // diff drive, fused, four- or one-wave: a turn per step beyond pi/4 -> sin / cos of every heading in full
    int batch;         // instances of a batch handle's launch (A.frame = their records, batch_view); 0 = a single handle
    BatchForm form;    // what the kernel serves (mppi_kernels.h): Single if and only if batch == 0
    bool shift;        // form >= Varied: shifted weights (ccv_mppi_batch_set_min_shift; the four- and one-wave kernels' SHIFT forms)
    bool lds_window;   // Plain: the window from LDS (false: CCV_MPPI_WINDOW=scalar)
};

// whether the one-wave kernel of a model has the form: the full-body kernel has no register left for the grid term (DESIGN.md
// section 10h; the kernel's own assert, mppi_rollout_solo.h).  make_plan() sends such a plan to the four-wave kernel.
constexpr bool has_one_wave_form(const int model, const BatchForm form) { return !(model == CCV_MPPI_FULL_BODY && form >= BatchForm::Grid); }

// K, H, ... come from the arguments themselves.  Plain: device noise in the fused iteration, else the controls of the buffer.
// Built: batches -- Plain, FourWave, OneWave, fused; ThreeWave -- not full body; OneWave -- fused.
void launch_rollout(const RolloutPlan& plan, const LaunchAt& at, const RolloutArgs& A, const Window& W);
void launch_sample(int model, hipStream_t stream, const RolloutArgs& A);

// ---- for the kernel units --------------------------------------------------------------------------------------------
template <class KERNEL>
inline void launch_at(KERNEL kernel, const dim3 grid, const dim3 block, const LaunchAt& at, const RolloutArgs& A, const Window& W) {
    if (at.ev_start) hipExtLaunchKernelGGL(kernel, grid, block, 0, at.stream, at.ev_start, at.ev_stop, 0, A, W);
    else hipLaunchKernelGGL(kernel, grid, block, 0, at.stream, A, W);
}
// workgroups of 64 samples: a single handle's K, or `batch` instances of it on one axis
inline dim3 blocks_of_64(const RolloutArgs& A, const int batch) { return dim3((unsigned)(batch ? batch : 1) * (unsigned)((A.K + 63) / 64)); }
// the plain kernel's grid: (workgroups per instance, instances)
inline dim3 blocks_plain(const RolloutArgs& A, const int batch) { return dim3((unsigned)((A.K + kBlock - 1) / kBlock), (unsigned)(batch ? batch : 1)); }

}  // namespace ccv

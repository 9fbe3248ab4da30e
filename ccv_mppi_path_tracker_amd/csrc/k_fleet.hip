// translation unit: the fleet forms of the batch prologue kernels (mppi_fleet.h).  A unit of its own:
// new instantiations beside existing kernels have changed those kernels' generated code before (section 10).  The update
// blocks and the prologue itself are the device functions k_update.hip's kernels are made of (mppi_update_device.h); what is
// new is fleet_step (mppi_fleet_device.h), in the prologue workgroup of every instance.
#include "mppi_fleet_device.h"

namespace ccv {

// k_advance_batch_varied with the fleet step: grid B, instance blockIdx.x, its command read from u*[b][0]
__global__ __launch_bounds__(kBatchAdvanceThreads) void k_advance_batch_fleet(const BatchAdvanceArgs G, BatchParams* P, const FleetArgs L) {
    const int b = (int)blockIdx.x;
    fleet_step(L, P, b);
    double* rec;
    const AdvanceArgs A = batch_advance_view<true>(G, b, rec, P);
    advance_body<kBatchAdvanceThreads, true>(A, A.nominal, rec);
    fleet_publish(L, G.frames, b);
}

// k_finalize_advance_batch_varied with the fleet step
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_fleet(FinalizeArgs I, const BatchAdvanceArgs G, BatchParams* P,
                                                                         const FleetArgs L) {
    finalize_advance_fleet<false>(I, G, P, L, RowSum<false>{});
}

// k_finalize_advance_batch_shift with the fleet step: the extra block forms the command with shift_scaled_sum2 as well
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_shift_fleet(FinalizeArgs F, const BatchAdvanceArgs G, BatchParams* P,
                                                                               const FleetArgs L) {
    finalize_advance_fleet<true>(F, G, P, L, RowSum<true>{P[blockIdx.y].lambda, G.K});
}

}  // namespace ccv

// translation unit: the fleet forms of the batch prologue kernels WITH prediction (ccv_mppi_batch_set_fleet_prediction; DESIGN.md
// section 10g): k_fleet.hip's three kernels with PRED -- every robot's velocity over the tick travels with its position through
// the double-buffered snapshot, and a selected neighbour's velocity goes into the velocity row of its disc, for the MOVING
// rollout kernels of the same tick.  A unit of its own: the kernels of k_fleet.hip stay as they are.
#include "mppi_fleet_device.h"

namespace ccv {

__global__ __launch_bounds__(kBatchAdvanceThreads) void k_advance_batch_fleet_pred(const BatchAdvanceArgs G, BatchParams* P, const FleetArgs L,
                                                                                   const FleetPredArgs V) {
    const int b = (int)blockIdx.x;
    fleet_step<true>(L, P, b, &V);
    double* rec;
    const AdvanceArgs A = batch_advance_view<true>(G, b, rec, P);
    advance_body<kBatchAdvanceThreads, true>(A, A.nominal, rec);
    fleet_publish<true>(L, G.frames, b, &G, &V);
}

__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_fleet_pred(FinalizeArgs I, const BatchAdvanceArgs G, BatchParams* P,
                                                                              const FleetArgs L, const FleetPredArgs V) {
    finalize_advance_fleet<false, true>(I, G, P, L, RowSum<false>{}, &V);
}

__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_shift_fleet_pred(FinalizeArgs F, const BatchAdvanceArgs G, BatchParams* P,
                                                                                    const FleetArgs L, const FleetPredArgs V) {
    finalize_advance_fleet<true, true>(F, G, P, L, RowSum<true>{P[blockIdx.y].lambda, G.K}, &V);
}

}  // namespace ccv

// Batch handles, fleet term (ccv_mppi_batch_resident_set_fleet): the robots of one resident batch keep
// clear of each other.  In front of every resident tick the prologue workgroup of instance y turns the fleet's positions into
// discs of instance y's own list -- after its n_static[y] discs of ccv_mppi_batch_set_obstacles, up to
// M_y = min(max_neighbours, CCV_MPPI_MAX_OBSTACLES - n_static[y]) discs (q_j, radius[y] + radius[j]) for the nearest other robots
// within `range` -- and writes the row count the OBST rollout kernels of the same tick read (BatchParams::n_obst).  The rollout
// kernels and the update arithmetic are untouched: the fleet forms of the three prologue kernels that take the parameter table
// are defined in k_fleet.hip, over the device functions of mppi_update_device.h.
//
// The snapshot: every position a tick uses is a pose at the start of that tick.  Other instances' prologue blocks move their
// frames in the same launch, so the positions come from a table of their own, xy[2][B][2]: tick n reads half n & 1 and block y
// writes its post-advance position into the other half.
#pragma once
#include "mppi_resident.h"

namespace ccv {

constexpr int kFleetMaxBatch = 1024;   // the positions of one half are staged in LDS: 16 KB

struct FleetArgs {
    const double* xy_in;       // [B][2]: every robot's position at the start of this tick
    double* xy_out;            // [B][2]: block y writes instance y's position after this tick's advance
    const double* radius;      // [B]
    const int32_t* n_static;   // [B]: instance y's discs of ccv_mppi_batch_set_obstacles, rows 0 .. n_static[y]-1 of its list
    double* obst;              // [B][CCV_MPPI_MAX_OBSTACLES][3]: the table BatchParams::obst points into
    double range2;             // range * range, rounded once on the host
    int32_t max_neighbours, B;
};

// Fleet prediction (ccv_mppi_batch_set_fleet_prediction): the velocities travel with the positions, v[2][B][2]
// double buffered like xy, and a selected neighbour's goes into the velocity row of its disc
struct FleetPredArgs {
    const double* v_in;    // [B][2]: every robot's velocity over the tick that made xy_in (zero where that tick did not move it)
    double* v_out;         // [B][2]: block y writes instance y's velocity over this tick
    double* obst_v;        // [B][CCV_MPPI_MAX_OBSTACLES][2]: the table BatchParams::obst_v points into
};

// k_advance_batch_varied, k_finalize_advance_batch_varied and k_finalize_advance_batch_shift with the fleet step in the
// prologue workgroup; P: the parameter table [B], whose n_obst the step writes
__global__ void k_advance_batch_fleet(BatchAdvanceArgs G, BatchParams* P, FleetArgs L);
__global__ void k_finalize_advance_batch_fleet(FinalizeArgs F, BatchAdvanceArgs G, BatchParams* P, FleetArgs L);
__global__ void k_finalize_advance_batch_shift_fleet(FinalizeArgs F, BatchAdvanceArgs G, BatchParams* P, FleetArgs L);
// ... and with prediction (k_fleet_pred.hip)
__global__ void k_advance_batch_fleet_pred(BatchAdvanceArgs G, BatchParams* P, FleetArgs L, FleetPredArgs V);
__global__ void k_finalize_advance_batch_fleet_pred(FinalizeArgs F, BatchAdvanceArgs G, BatchParams* P, FleetArgs L, FleetPredArgs V);
__global__ void k_finalize_advance_batch_shift_fleet_pred(FinalizeArgs F, BatchAdvanceArgs G, BatchParams* P, FleetArgs L, FleetPredArgs V);

}  // namespace ccv

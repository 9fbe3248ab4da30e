// What a node publishes per robot, for every instance of a batch handle at once (ccv_mppi_batch_read_best_candidates /
// _read_optimal_paths): the lowest-cost samples of every instance with their rollouts, and the plant
// model rolled through every instance's u*.  Both read what the tick left on the device -- costs, states, records, warm starts --
// and write only their own output; no rollout, prologue or update kernel knows of them.  The kernels are k_feed.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccv {

// One launch: grid B, kBlock threads.  Workgroup b selects and orders the N lowest costs of cost[b * kpad .. + K)
// (select_lowest, mppi_select.h: by (select_key, sample index)), writes their local sample indices and costs, then gathers their
// N * H states.  Columns K .. kpad - 1 of an instance are never read.
struct BestArgs {
    const double* cost;   // [B * kpad]
    const double* xs;     // [H][pitch], pitch = B * kpad (read only when xy_out is set)
    const double* ys;
    int32_t* idx_out;     // [B][N]
    double* cost_out;     // [B][N], or null
    double* xy_out;       // [B][N][H][2], or null
    int32_t K, kpad, pitch, H, N;   // 1 <= N <= min(K, kSelectMax)
};
__global__ void k_best_candidates(BestArgs A);

// One lane per instance, grid ceil(B / kBlock): the plant of k_advance / ccv_mppi_plant_step applied H - 1 times from the pose
// and dt in the instance's record (BatchHead, mppi_kernels.h) with the rows of its u*; out row i = (x, y, yaw) BEFORE control
// step i, as MPPIBase::optimal_path().
struct PathArgs {
    const double* rec;       // [B][rec_doubles]
    const double* nominal;   // u* [B][R], R = (H - 1) * udim
    double* out;             // [B][H - 1][3]
    int32_t B, H, R, model, rec_doubles;
};
__global__ void k_optimal_paths(PathArgs A);

}  // namespace ccv

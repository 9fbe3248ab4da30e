// Device-resident closed loop: the per-tick prologue of the reference's run() loop on the GPU, so that consecutive MPPI
// iterations need nothing from the host but their launches.
//
//   k_advance   (optional) the commanded motion u*[0] applied to the pose for one period -- the kinematic plant of the
//               closed-loop harness, the Euler model of predict_NextState() (dd:104-109, sd:120-125, fb:445-452 pose part)
//               get_CurrentIndex()   nearest path pose inside the 100 m gate      dd:126-140  sd:142-156  fb:335-349
//               calc_RefPath()       window of H poses, stride v_ref*dt/resolution dd:156-181  sd:172-197  fb:365-392
//               + the distance coefficients of the window relative to the pose (window_coeffs() in ccv_mppi_capi.hip)
//
// One workgroup; the path (a few hundred to a few thousand poses) is scanned by its 1024 threads and the (distance, index)
// pairs are reduced so that the result is the one the reference's serial scan gives: the lowest index among the poses at
// the smallest distance, 0 when none is inside the gate.  x_ref / y_ref / index and the coefficients are bit-identical to
// ccv_mppi_calc_ref_path() + window_coeffs() on the host (same operations, no contraction); the plant uses fast_sincos(),
// which ccv_mppi_plant_step() restates operation by operation on the host; yaw_ref0 comes from the device atan2 and may
// differ from libm's in the last place (only fb:408 reads it).
//
// This header: the argument structs and the kernels' declarations, for the host units that fill and launch them
// (capi_resident.hip, capi_batch.hip).  The kernels are defined in k_update.hip.
#pragma once
#include "fast_trig.h"
#include "mppi_update.h"

namespace ccv {

struct AdvanceArgs {
    ResidentFrame* frame;
    const double* path_x;
    const double* path_y;
    const double* nominal;   // u* (row n = t*u_dim + d): the command is rows 0..u_dim-1
    double* trace;           // [trace_cap][6]: pose (5) and index after each launch (ring), or null
    double dt, v_ref, resolution;
    int32_t n_path, H, model, advance, trace_cap;
};

constexpr int kAdvanceThreads = 1024;   // one workgroup; a path of a few thousand poses is one or two batches of loads per thread

__global__ void k_advance(AdvanceArgs A);   // one workgroup of kAdvanceThreads

// the update of tick i and the prologue of tick i+1 in one launch: grid finalize_blocks(R) + 1
__global__ void k_finalize_advance(FinalizeArgs F, AdvanceArgs A);

// ---- batch handles (ccv_mppi_batch_resident_*): the same prologue for B instances, one workgroup each ---------------------
// Instance b has a path of its own (a slice of one array of all paths), a ResidentFrame of its own (pose, index, window,
// step count; its W is not used) and a trace ring of its own.  The prologue writes the instance's batch record -- the block
// batch_enqueue() fills on the host and the batched rollout reads (BatchHead + window) -- so that a batched resident tick
// needs no host data.
struct BatchInstance {
    int64_t path_off;    // first pose of the instance's path in BatchAdvanceArgs::path
    int32_t n_path, pad;
    double resolution;
    uint32_t seed_lo, seed_hi;   // the instance's noise key (ccv_mppi_batch_resident_set_poses)
};

struct BatchAdvanceArgs {
    ResidentFrame* frames;          // [B]
    double* rec;                    // [B][batch_record_doubles(H)]
    const BatchInstance* inst;      // [B]
    const double* path;             // [2][n_total]: every instance's x, back to back, then every instance's y
    double* nominal;                // u* [B][R]
    double* trace;                  // [B][trace_cap][6]
    int64_t n_total;
    double dt, inv_dt, v_ref;       // (inv_dt: 1 / dt, correctly rounded on the host, as batch_enqueue writes it)
    int32_t H, R, K, kpad, model, advance, trace_cap;
};

constexpr int kBatchAdvanceThreads = kBlock;   // (the lexicographic reduction is exact: any width gives the same index)

// grid B: instance blockIdx.x, its command read from u*[b][0]
__global__ void k_advance_batch(BatchAdvanceArgs G);
// the batched k_finalize_advance: grid (finalize_blocks(R) + 1, B)
__global__ void k_finalize_advance_batch(FinalizeArgs F, BatchAdvanceArgs G);
// the two prologue kernels of a batch with per-instance parameters (ccv_mppi_batch_set_params): P = the parameter table [B]
__global__ void k_advance_batch_varied(BatchAdvanceArgs G, const BatchParams* P);
__global__ void k_finalize_advance_batch_varied(FinalizeArgs F, BatchAdvanceArgs G, const BatchParams* P);
// ... and of a batch in shifted-weight mode (k_finalize_batch_shift's update; its prologue is k_advance_batch_varied)
__global__ void k_finalize_advance_batch_shift(FinalizeArgs F, BatchAdvanceArgs G, const BatchParams* P);

}  // namespace ccv

// The shared vocabulary of the MPPI rollout kernels for gfx950 (MI355X) and of the host code that launches them: constants,
// the MODE_* / SRC_* enums, the argument structs (Window, ResidentFrame, BatchHead / BatchParams / GridRow, BatchForm,
// RolloutArgs) and a workgroup's view of them (batch_view, rollout_view, stage_window).  No kernel and no cost arithmetic.
// Hand-written HIP, wave64, one sample per lane; the kernels over these types:
//
//   k_rollout_cost   sampling() + predict_States() + calc_Cost()/calc_MinDistance() + exp   (dd:81-124,183-221;
//                    sd:97-140,199-237; fb:394-424,445-520)  -- the plain family, mppi_rollout_plain.h; the cooperative
//                    families: mppi_rollout_r4.h, mppi_rollout_r3.h, mppi_rollout_pc.h, mppi_rollout_solo.h
//   k_update_partials / k_finalize / k_apply_partials    calc_Weights() normalisation + determine_OptimalSolution()
//                    (dd:216-237, sd:232-255, fb:437-326)  -- in mppi_update.h
//   k_sample         stand-alone sampling() for the stage-wise ABI  -- mppi_rollout_plain.h
//   k_gather_xy      strided read-back feeding publish_CandidatePath() (dd:265-294)
//
// Data layout in HBM (all fp64, k fastest => every store/load of a wave is one contiguous 512-byte run):
//   u    [(H-1)*u_dim][pitch]   row n = t*u_dim + d  clamped sample controls (sample[i].v_[t] ... in the reference); written by
//                               the stage-wise calls and the plain kernel only -- the fused iteration stores, in its place,
//   z    [(H-1)*u_dim][pitch]   fp32: the N(0,1) variate each control was made from, with the warm start it was made around
//                               (nominal_used): u = clamp(double(z) * sigma + u*[n]) is re-derived, bit for bit, where it is
//                               needed (epilogue, ccv_mppi_read_controls, k_materialize_controls) -- half the bytes to store and
//                               to re-read
//   xs,ys[H][pitch]             sample[i].x_[t], sample[i].y_[t]
//   cost [pitch], w [pitch]     per-sample cost and unnormalised weight exp(-cost/lambda)
//   nominal [(H-1)*u_dim]       optimal_solution controls (resident warm start)
// pitch = K rounded up to 64.  Compiled with -ffp-contract=off: a*b+c is fused only where fma() is written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ccv_mppi.h"

#if defined(CCV_DIAG)
#include "mppi_diag.h"   // in-kernel time stamps of the diagnostic builds (tools/ablate.py, tools/stamps_r4.py)
#else
#define CCV_DIAG_STAMP(A, slot) do {} while (0)   // a product build contains nothing of the diagnostics
#define CCV_DIAG_STAMP_VALUE(A, slot, value) do {} while (0)
#endif

namespace ccv {

constexpr int kMaxH = CCV_MPPI_MAX_HORIZON;
constexpr int kTU = 8;        // time steps per register block (kTU*u_dim is a multiple of 4 normals for every model)
constexpr int kBlock = 256;   // 4 waves: one per SIMD of a CU
constexpr int kChunk = 2048;  // samples per k_update_partials block
constexpr int kPcSamples = 64;   // samples per block of the cooperative kernels: one per lane (mppi_rollout_*.h)
constexpr int kPartialMin = 4;   // fewest control steps of a horizon's last block that is made as a masked batch (pc_produce_batched,
                                 // PARTIAL, mppi_produce.h: why 4); the launcher picks the four-wave kernel's TAIL form by it
constexpr int kMaxObst = CCV_MPPI_MAX_OBSTACLES;   // discs per instance (mppi_cost_terms.h)

enum : int { MODE_FUSED = 0, MODE_ROLLOUT = 1, MODE_COST = 2 };
//   MODE_FUSED    device Philox noise, controls + states stored, cost + weight   (ccv_mppi_iterate*)
//   MODE_ROLLOUT  controls read from HBM, states stored, no cost                  (ccv_mppi_rollout)
//   MODE_COST     controls read from HBM, nothing stored but cost + weight        (ccv_mppi_weights)

enum : int { SRC_PHILOX = 0, SRC_BUFFER = 1 };

__host__ __device__ constexpr int udim_of(int model) { return model == 0 ? 2 : (model == 1 ? 3 : 5); }

// Window coefficients: squared distance to window point j is |p|^2 + a_j*px + b_j*py + c_j with p relative to the
// current pose.  Travels in the kernel-argument segment (wave-uniform => scalar loads).
struct Window {
    double a[kMaxH];
    double b[kMaxH];
    double c[kMaxH];
};

// Device-resident closed loop (k_advance, mppi_resident.h): the pose, the window built from it and its distance coefficients stay
// in HBM; a rollout launched with RolloutArgs::frame set takes x0, yaw_ref0 and the window from here instead of from its
// kernel arguments.
struct ResidentFrame {
    double x0[5];      // x, y, yaw[, roll, pitch]
    double yaw_ref0;   // yaw_ref[0] of calc_RefPath() (fb:408 is its only reader)
    int32_t index;     // current_index_ (get_CurrentIndex())
    int32_t steps;     // k_advance launches so far
    Window W;
    double x_ref[kMaxH], y_ref[kMaxH];
};

// Batch handles (ccv_mppi_batch_*): B independent problems of K samples each share one configuration and lie on ONE sample
// axis of B * Kpad columns (Kpad = K rounded up to 64) in the layout above, so no workgroup of 64 samples straddles two
// instances.  What differs per instance travels in a record in device memory, one per instance, batch_record_doubles(H)
// doubles apart: a BatchHead (two 64-byte lines), then the window coefficients a[H], b[H], c[H].  A batched rollout is
// launched with RolloutArgs::frame pointing at record 0 and takes its instance's record in batch_view() below.
struct BatchParams;
struct BatchHead {
    double x0[5];
    double yaw_ref0;
    double dt, inv_dt;
    uint32_t seed_lo, seed_hi;
    int32_t K, k_offset;        // b * Kpad + K and -b * Kpad (see batch_view)
    const double* nominal;      // the instance's warm start
    const BatchParams* params;  // the instance's row of the parameter table (ccv_mppi_batch_set_params; VARIED kernels only)
};
// Per-instance controller parameters of a batch handle (ccv_mppi_batch_set_params): one row per instance, three 64-byte lines,
// the RolloutArgs fields fill_args() forms from a configuration -- ROLL_OFF's zero weights and the fast-clamp test included.
// A VARIED kernel takes its instance's row in batch_view() and is the single handle's code from there on.
// obst / n_obst / w_obs (ccv_mppi_batch_set_obstacles; OBST kernels only): the instance's discs, rows (ox, oy, r) of a device
// table, and the weight of their penalty; null / 0 / 0 without obstacles.
// obst_v (ccv_mppi_batch_set_obstacle_velocities; MOVING kernels only): the discs' velocities, rows (vx, vy) of a device table
// [B][32][2] beside the discs'; null while no velocities are set.  Every row of a non-null table is defined: zero unless given.
// grid (ccv_mppi_batch_set_grids; GRID kernels only): the instance's row of the occupancy-grid table; null without a map.
struct GridRow;
struct alignas(64) BatchParams {
    double sigma, lambda, v_ref;
    double umin[5], umax[5];
    double w_path, w_v, w_zmp, w_rollv, w_back, w_yaw;
    int32_t fast_clamp, n_obst;
    const double* obst;
    double w_obs;
    const double* obst_v;
    const GridRow* grid;
};
static_assert(sizeof(BatchParams) == 192, "three 64-byte lines per instance");
// One instance's occupancy grid (GRID kernels): a 64-byte row of a device table [B].  The map is nx x ny
// cells of float, row-major with x fastest, its corner at (origin_x, origin_y) in world coordinates; inv = RN(1 / resolution),
// formed on the host; `outside` is the value of everything that is not in a cell.  nx, ny in [1, 32 768], nx * ny <= 2^26.
struct alignas(64) GridRow {
    double origin_x, origin_y, inv, w;
    const float* cells;
    int32_t nx, ny;
    float outside;
};
static_assert(sizeof(GridRow) == 64, "one 64-byte line per instance");
// What a rollout kernel serves, as one ordered value: every rung is the one before it plus one thing, so a kernel (template
// parameter FORM of k_rollout_r4, k_rollout_solo, k_rollout_cost), a launch (RolloutPlan::form, mppi_launch.h) and a handle
// (batch_form(), capi_batch.hip) each name a rung, and "has X" is FORM >= X.
//   Single  a single handle: no records
//   Batch   + the instances' records (BatchHead, batch_view below)
//   Varied  + the per-instance parameter table (BatchParams above)
//   Obst    + the instance's disc obstacles (obst_stage, obst_term: mppi_cost_terms.h)
//   Moving  + the discs' velocities (obst_stage_moving, obst_term_moving: mppi_cost_terms.h)
//   Grid    + the instance's occupancy grid (GridRow above, grid_tap: mppi_cost_terms.h)
// The shifted weights (SHIFT, pc_shifted_weight in mppi_epilogue.h) are the one independent bit: on any rung from Varied up.
enum class BatchForm : int { Single, Batch, Varied, Obst, Moving, Grid };
constexpr int kBatchHeadDoubles = 16;
__host__ __device__ constexpr int batch_record_doubles(int H) { return kBatchHeadDoubles + ((3 * H + 7) & ~7); }

struct RolloutArgs {
    double x0[5];
    double dt;
    double yaw_ref0;
    double sigma, lambda, v_ref;
    double umin[5], umax[5];
    double w_path, w_v, w_zmp, w_rollv, w_back, w_yaw;
    double fb_mass, fb_L, fb_Ixx, fb_gz;  // fb.h:212-216, fb:86-91, fb.h:30
    double inv_dt;                        // 1 / dt, correctly rounded on the host: div_uniform(), mppi_device_util.h
    uint32_t seed_lo, seed_hi, iter_lo, iter_hi;
    int32_t K, pitch, H, k_offset;
    int32_t steer_off, store_u, store_xy, do_cost;
    const double* __restrict__ nominal;
    double* u;
    float* z;                 // fused iteration: the normals, in place of u (see the layout comment at the top)
    double* nominal_used;     // ... and the warm start they were made around (written by workgroup 0)
    double* xs;
    double* ys;
    double* cost;
    double* w;
    double* partial;    // fused update: [(R+1)][nparts] per-workgroup sums of w and w*u (null: not fused)
    double* statpart;   // [nparts][3]: min cost, max cost, zero-weight count
    int32_t nparts, fuse_update;
    int32_t prio_rotate, cu_count;   // k_rollout_pc / k_rollout_r3: see pc_rotate_priority()
    int32_t prune, fast_clamp;       // exact pruning of the window in the distance loop (pc_prune_window); 0 = off.  fast_clamp: clampd_fast() allowed (host side: sigma finite, umin <= umax)
    // deferred ccv_mppi_apply_partials_enqueue (K sharded over devices): when set, the warm start is pending_vec[1..] /
    // pending_vec[0]; every workgroup forms it while staging u* in LDS and workgroup 0 writes it (and sum w) back
    const double* pending_vec;
    double* nominal_w;
    double* stats_w;
    const ResidentFrame* frame;   // device-resident pose and window (null: x0, yaw_ref0 and the Window argument)
    unsigned long long* dbg;   // diagnostic builds only (-DCCV_DIAG, mppi_diag.h): the stamp buffer; null otherwise
};

// Every 64-byte line of the RolloutArgs block of the kernel arguments, requested at once.  The host wrote the block into
// device memory a moment ago and every launch starts with an invalidated scalar cache, so the first use of a field is a miss
// all the way to HBM (0.4 us on an idle chip, about 1 us on a busy one) -- and the compiler loads the fields where they are
// first needed: three to four of those latencies in a row before a wave has done anything (entry -> first arguments ->
// pointers -> loop bounds).  One dword of each line, all in flight together, then one wait: the lines are in the scalar
// cache, every later load of a field hits.
__device__ __forceinline__ void touch_rollout_args() {
    typedef const uint32_t __attribute__((address_space(4))) * ConstArgWords;
    ConstArgWords ka = (ConstArgWords)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t t = 0;
#pragma unroll
    for (int off = 0; off < (int)sizeof(RolloutArgs); off += 64) t |= ka[off / 4];
    asm volatile("" ::"s"(t));
}

// the kernel arguments with the resident pose substituted (wave-uniform scalar loads)
__device__ __forceinline__ RolloutArgs with_resident_pose(const RolloutArgs& Ak) {
    RolloutArgs A = Ak;
    if (Ak.frame) {
#pragma unroll
        for (int i = 0; i < 5; ++i) A.x0[i] = Ak.frame->x0[i];
        A.yaw_ref0 = Ak.frame->yaw_ref0;
    }
    return A;
}

// Instance `inst` of a batched launch as a single handle of its own: pose, dt, 1 / dt, yaw_ref0, the noise key and its slice
// of the warm start from its record, the window from the record too (stage_window<true>, r4_stage_issue<..., true>).  The
// sample index stays the global column k = inst * Kpad + local k: K and k_offset are shifted by inst * Kpad instead (the
// host writes them into the record), so that `k < K` masks the lanes past the instance's own K and k_offset + k is the
// LOCAL index, the counter word of noise_spec.h.  The partials stay [(R+1)][nparts] with nparts = B * the instance's
// workgroups: column blockIdx.x, each instance's columns contiguous (k_finalize_batch).  Workgroup 0 of the launch
// (instance 0) writes nominal_used; the batch has no read-back of the controls that would need the other instances'.
// VARIED: the controller parameters (sigma, lambda, v_ref, bounds, weights, the clamp form) from the instance's row of the
// parameter table too, whose address the head holds -- read through the constant address space as well.
template <bool VARIED = false>
__device__ __forceinline__ RolloutArgs batch_view(const RolloutArgs& Ak, const int inst) {
    RolloutArgs A = Ak;
    const double* rec = reinterpret_cast<const double*>(Ak.frame) + (size_t)inst * batch_record_doubles(Ak.H);
    // (read through the constant address space, like the kernel arguments: the compiler may load a field again where it is
    //  used instead of holding it in registers from entry to exit -- held, they pushed the four-wave kernel into more spills)
    typedef const BatchHead __attribute__((address_space(4))) * ConstHead;
    const auto& hd = *(ConstHead)(const void*)rec;
#pragma unroll
    for (int i = 0; i < 5; ++i) A.x0[i] = hd.x0[i];
    A.yaw_ref0 = hd.yaw_ref0;
    A.dt = hd.dt;
    A.inv_dt = hd.inv_dt;
    A.seed_lo = hd.seed_lo;
    A.seed_hi = hd.seed_hi;
    A.frame = reinterpret_cast<const ResidentFrame*>(rec);
    A.K = hd.K;
    A.k_offset = hd.k_offset;
    A.nominal = hd.nominal;
    if constexpr (VARIED) {
        typedef const BatchParams __attribute__((address_space(4))) * ConstParams;
        const auto& P = *(ConstParams)(const void*)hd.params;
        A.sigma = P.sigma;
        A.lambda = P.lambda;
        A.v_ref = P.v_ref;
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            A.umin[d] = P.umin[d];
            A.umax[d] = P.umax[d];
        }
        A.w_path = P.w_path;
        A.w_v = P.w_v;
        A.w_zmp = P.w_zmp;
        A.w_rollv = P.w_rollv;
        A.w_back = P.w_back;
        A.w_yaw = P.w_yaw;
        A.fast_clamp = P.fast_clamp;
    }
    return A;
}
// the kernel arguments of a workgroup of 64 samples: batched (instance = workgroup / workgroups per instance) or not
template <int MODEL, bool BATCH, bool VARIED = false>
__device__ __forceinline__ RolloutArgs rollout_view(const RolloutArgs& Ak) {
    if constexpr (BATCH) return batch_view<VARIED>(Ak, (int)blockIdx.x / ((Ak.K + 63) >> 6));
    else return with_resident_pose(Ak);
}

// window coefficients -> LDS, padded to a multiple of 4 points with c = +inf (never the minimum)
template <bool BATCH = false, class SH>
__device__ __forceinline__ void stage_window(const RolloutArgs& A, const Window& Wk, SH& sh, int nthreads,
                                             const int tid = threadIdx.x) {   // (tid: 0 .. nthreads-1 over the staging threads)
    const int H = A.H, H4 = (H + 3) & ~3;
    if constexpr (BATCH) {   // (batch_view: the instance's record)
        const double* win = reinterpret_cast<const double*>(A.frame) + kBatchHeadDoubles;
        for (int j = tid; j < H4; j += nthreads) {
            sh.ab[j] = j < H ? make_double2(win[j], win[H + j]) : make_double2(0.0, 0.0);
            sh.c[j] = j < H ? win[2 * H + j] : INFINITY;
        }
    } else if (A.frame) {
        const Window& W = A.frame->W;
        for (int j = tid; j < H4; j += nthreads) {
            sh.ab[j] = j < H ? make_double2(W.a[j], W.b[j]) : make_double2(0.0, 0.0);
            sh.c[j] = j < H ? W.c[j] : INFINITY;
        }
    } else {
        for (int j = tid; j < H4; j += nthreads) {
            sh.ab[j] = j < H ? make_double2(Wk.a[j], Wk.b[j]) : make_double2(0.0, 0.0);
            sh.c[j] = j < H ? Wk.c[j] : INFINITY;
        }
    }
}

}  // namespace ccv

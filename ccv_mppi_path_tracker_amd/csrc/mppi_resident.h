// Device-resident closed loop: the per-tick prologue of the reference's run() loop on the GPU, so that consecutive MPPI
// iterations need nothing from the host but their launches.
//
//   k_advance   (optional) the commanded motion u*[0] applied to the pose for one period -- the kinematic plant of the
//               closed-loop harness, the Euler model of predict_NextState() (dd:104-109, sd:120-125, fb:445-452 pose part)
//               get_CurrentIndex()   nearest path pose inside the 100 m gate      dd:126-140  sd:142-156  fb:335-349
//               calc_RefPath()       window of H poses, stride v_ref*dt/resolution dd:156-181  sd:172-197  fb:365-392
//               + the distance coefficients of the window relative to the pose (fill_window() in ccv_mppi_capi.hip)
//
// One workgroup; the path (a few hundred to a few thousand poses) is scanned by its 1024 threads and the (distance, index)
// pairs are reduced so that the result is the one the reference's serial scan gives: the lowest index among the poses at
// the smallest distance, 0 when none is inside the gate.  x_ref / y_ref / index and the coefficients are bit-identical to
// ccv_mppi_calc_ref_path() + fill_window() on the host (same operations, no contraction); the plant uses fast_sincos(),
// which ccv_mppi_plant_step() restates operation by operation on the host; yaw_ref0 comes from the device atan2 and may
// differ from libm's in the last place (only fb:408 reads it).
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

// NT threads of one workgroup; cmd: the command u*[0][0 .. u_dim) (read only when A.advance).  BATCH: the window
// coefficients go into the instance's batch record `rec` (BatchHead + a[H], b[H], c[H]) instead of A.frame->W, and the pose
// and yaw_ref0 into its head as well -- what batch_enqueue() writes on the host for the same pose and window.
template <int NT, bool BATCH = false>
__device__ __forceinline__ void advance_body(const AdvanceArgs& A, const double* cmd, double* rec = nullptr) {
    __shared__ double s_d[NT / 64];
    __shared__ int s_i[NT / 64];
    __shared__ int s_start;
    ResidentFrame& F = *A.frame;
    // ---- pose (every thread computes it: wave-uniform, no hand-off)
    double x = F.x0[0], y = F.x0[1], yaw = F.x0[2], roll = F.x0[3], pitch = F.x0[4];
    if (A.advance) {
        const double v = cmd[0], w = cmd[1];
        const double heading = A.model == CCV_MPPI_DIFF_DRIVE ? yaw : yaw + cmd[2];
        double sn, cs;
        fast_sincos(heading, sn, cs);
        x = x + v * cs * A.dt;
        y = y + v * sn * A.dt;
        yaw = rebase_angle(yaw + w * A.dt);
        if (A.model == CCV_MPPI_FULL_BODY) {
            roll = rebase_angle(roll + cmd[3] * A.dt);
            pitch = rebase_angle(pitch + cmd[4] * A.dt);
        }
    }
    // ---- get_CurrentIndex(): strict '<' against a running minimum that starts at the 100 m gate
    double best_d = 100.0;
    int best_i = -1;
    constexpr int kBatch = 4;   // loads in flight per thread: the scan is a chain of memory latencies otherwise
    for (int i0 = threadIdx.x; i0 < A.n_path; i0 += NT * kBatch) {
        double qx[kBatch], qy[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int i = min(i0 + b * NT, A.n_path - 1);
            qx[b] = A.path_x[i];
            qy[b] = A.path_y[i];
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int i = i0 + b * NT;
            const double ex = x - qx[b], ey = y - qy[b];
            const double d = sqrt(ex * ex + ey * ey);
            if (i < A.n_path && d < best_d) {   // (ascending i within a thread: the first of equal distances stays)
                best_d = d;
                best_i = i;
            }
        }
    }
    // (distance, index) minimum, lexicographic: the smallest distance, and among equal distances the smallest index --
    // what the serial scan's strict '<' keeps.  Two wave reductions per level (DPP), one LDS hand-off between the levels.
    auto lexmin = [](double d, int i, double& d_out, int& i_out) {
        const double dm = wave_min(d);                                   // (no candidate: d = 100, the gate)
        const double im = wave_min((i >= 0 && d == dm) ? (double)i : 1.0e300);
        d_out = dm;
        i_out = im < 1.0e299 ? (int)im : -1;
    };
    double wd;
    int wi;
    lexmin(best_d, best_i, wd, wi);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_d[wave] = wd;
        s_i[wave] = wi;
    }
    __syncthreads();   // (also: every thread has read the old pose)
    if (wave == 0) {
        constexpr int NW = NT / 64;
        const double d2 = lane < NW ? s_d[lane] : 100.0;
        const int i2 = lane < NW ? s_i[lane] : -1;
        double fd;
        int fi;
        lexmin(d2, i2, fd, fi);
        if (lane == 0) s_start = fi < 0 ? 0 : fi;
    }
    __syncthreads();
    const int start = s_start;
    // ---- calc_RefPath(): the index is the truncation of a double; past the end the final pose repeats
    const double stride = A.v_ref * A.dt / A.resolution;
    for (int i = threadIdx.x; i < A.H; i += NT) {
        const int idx = (int)(start + i * stride);   // (the host admits 0 < dt < inf only: idx >= 0)
        const int src = idx < A.n_path ? idx : A.n_path - 1;
        const double xr = A.path_x[src], yr = A.path_y[src];
        F.x_ref[i] = xr;
        F.y_ref[i] = yr;
        const double xl = xr - x, yl = yr - y;
        if constexpr (BATCH) {
            double* win = rec + kBatchHeadDoubles;
            win[i] = -2.0 * xl;
            win[A.H + i] = -2.0 * yl;
            win[2 * A.H + i] = xl * xl + yl * yl;
        } else {
            F.W.a[i] = -2.0 * xl;
            F.W.b[i] = -2.0 * yl;
            F.W.c[i] = xl * xl + yl * yl;
        }
    }
    if (threadIdx.x == 0) {
        const int i1 = (int)(start + 1 * stride), i0 = (int)(start + 0 * stride);
        const int s1 = i1 < A.n_path ? i1 : A.n_path - 1, s0 = i0 < A.n_path ? i0 : A.n_path - 1;
        const double yaw_ref0 = atan2(A.path_y[s1] - A.path_y[s0], A.path_x[s1] - A.path_x[s0]);
        F.yaw_ref0 = yaw_ref0;
        if constexpr (BATCH) {
            BatchHead* hd = reinterpret_cast<BatchHead*>(rec);
            hd->x0[0] = x;
            hd->x0[1] = y;
            hd->x0[2] = yaw;
            hd->x0[3] = roll;
            hd->x0[4] = pitch;
            hd->yaw_ref0 = yaw_ref0;
        }
        F.x0[0] = x;
        F.x0[1] = y;
        F.x0[2] = yaw;
        F.x0[3] = roll;
        F.x0[4] = pitch;
        F.index = start;
        const int n = F.steps;
        F.steps = n + 1;
        if (A.trace) {
            double* t = A.trace + (size_t)(n % A.trace_cap) * 6;
            t[0] = x;
            t[1] = y;
            t[2] = yaw;
            t[3] = roll;
            t[4] = pitch;
            t[5] = (double)start;
        }
    }
}

__global__ __launch_bounds__(kAdvanceThreads) void k_advance(const AdvanceArgs A) { advance_body<kAdvanceThreads>(A, A.nominal); }

// The update of tick i and the prologue of tick i+1 in ONE launch (the closed loop then costs two launches per tick, not
// three): blocks 0 .. finalize_blocks(R)-1 are k_finalize; one more block forms the command u*[0][d] = V_d / S from the same
// partial sums in the same order (the same bits the finalize waves write into the warm start -- it cannot wait for them)
// and runs the prologue with it.
__global__ __launch_bounds__(kBlock) void k_finalize_advance(const FinalizeArgs F, const AdvanceArgs A) {
    if ((int)blockIdx.x < finalize_blocks(F.R)) {
        finalize_rows(F, (size_t)F.nchunks);
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (A.advance) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ud = udim_of(A.model);
        for (int d = wv; d < ud; d += kBlock / 64) {
            double s, v;
            lane_partial_sum2(F.partial + (size_t)F.R * F.nchunks, F.partial + (size_t)d * F.nchunks, F.nchunks, lane, s, v);
            s = wave_sum(s);
            v = wave_sum(v);
            if (lane == 0) cmd[d] = v / s;
        }
    }
    __syncthreads();
    advance_body<kBlock>(A, cmd);
}

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

// instance b's view of the batch: its AdvanceArgs, and the fields of its record that do not depend on the pose.  VARIED
// (per-instance parameters, P = the table of ccv_mppi_batch_set_params): the window stride takes the instance's v_ref, and the
// record's head the address of the instance's row, which the VARIED rollout kernels read (batch_view)
template <bool VARIED = false>
__device__ __forceinline__ AdvanceArgs batch_advance_view(const BatchAdvanceArgs& G, const int b, double*& rec,
                                                          const BatchParams* P = nullptr) {
    const BatchInstance in = G.inst[b];
    AdvanceArgs A;
    A.frame = G.frames + b;
    A.path_x = G.path + in.path_off;
    A.path_y = G.path + G.n_total + in.path_off;
    A.nominal = G.nominal + (size_t)b * G.R;
    A.trace = G.trace + (size_t)b * G.trace_cap * 6;
    A.dt = G.dt;
    if constexpr (VARIED) A.v_ref = P[b].v_ref;
    else A.v_ref = G.v_ref;
    A.resolution = in.resolution;
    A.n_path = in.n_path;
    A.H = G.H;
    A.model = G.model;
    A.advance = G.advance;
    A.trace_cap = G.trace_cap;
    rec = G.rec + (size_t)b * batch_record_doubles(G.H);
    if (threadIdx.x == 0) {
        BatchHead* hd = reinterpret_cast<BatchHead*>(rec);
        hd->dt = G.dt;
        hd->inv_dt = G.inv_dt;
        hd->seed_lo = in.seed_lo;
        hd->seed_hi = in.seed_hi;
        hd->K = b * G.kpad + G.K;
        hd->k_offset = -b * G.kpad;
        hd->nominal = G.nominal + (size_t)b * G.R;
        if constexpr (VARIED) hd->params = P + b;
    }
    return A;
}

// grid B: instance blockIdx.x, its command read from u*[b][0]
__global__ __launch_bounds__(kBatchAdvanceThreads) void k_advance_batch(const BatchAdvanceArgs G) {
    double* rec;
    const AdvanceArgs A = batch_advance_view(G, (int)blockIdx.x, rec);
    advance_body<kBatchAdvanceThreads, true>(A, A.nominal, rec);
}

// The batched k_finalize_advance: grid (finalize_blocks(R) + 1, B).  Blocks x < finalize_blocks(R) are k_finalize_batch
// (fused partials) for instance y; block x = finalize_blocks(R) forms instance y's command from the instance's own partial
// columns in k_finalize_batch's order (the bits its waves write into u*[y][0]) and runs the instance's prologue with it.
template <bool VARIED = false>
__device__ __forceinline__ void finalize_advance_batch(FinalizeArgs F, const BatchAdvanceArgs& G, const BatchParams* P = nullptr) {
    const size_t b = blockIdx.y;
    const size_t stride = (size_t)gridDim.y * F.nchunks;
    F.partial += b * F.nchunks;
    if ((int)blockIdx.x < finalize_blocks(F.R)) {
        F.statpart += b * (size_t)F.nchunks * 3;
        F.nominal += b * F.R;
        F.vec += b * (size_t)(F.R + 1);
        F.stats += b * 4;
        finalize_rows(F, stride);   // (no mailbox: a deferred update is never a blocking call's)
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (G.advance) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ud = udim_of(G.model);
        for (int d = wv; d < ud; d += kBlock / 64) {
            double s, v;
            lane_partial_sum2(F.partial + (size_t)F.R * stride, F.partial + (size_t)d * stride, F.nchunks, lane, s, v);
            s = wave_sum(s);
            v = wave_sum(v);
            if (lane == 0) cmd[d] = v / s;
        }
    }
    __syncthreads();
    double* rec;
    const AdvanceArgs A = batch_advance_view<VARIED>(G, (int)b, rec, P);
    advance_body<kBlock, true>(A, cmd, rec);
}
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch(FinalizeArgs F, const BatchAdvanceArgs G) {
    finalize_advance_batch(F, G);
}

// the two prologue kernels of a batch with per-instance parameters (ccv_mppi_batch_set_params): P = the parameter table [B]
__global__ __launch_bounds__(kBatchAdvanceThreads) void k_advance_batch_varied(const BatchAdvanceArgs G, const BatchParams* P) {
    double* rec;
    const AdvanceArgs A = batch_advance_view<true>(G, (int)blockIdx.x, rec, P);
    advance_body<kBatchAdvanceThreads, true>(A, A.nominal, rec);
}
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_varied(FinalizeArgs F, const BatchAdvanceArgs G,
                                                                           const BatchParams* P) {
    finalize_advance_batch<true>(F, G, P);
}

}  // namespace ccv

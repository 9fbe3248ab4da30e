// The device functions of the update and of the resident prologue that more than one translation unit instantiates: the
// packet store, the row sums of an update wave in both weight modes (RowSum, finalize_rows), the prologue of the
// device-resident loop (advance_body), a batch instance's view of it (batch_advance_view) and the command of a fused
// update-and-prologue launch (form_command).  k_update.hip defines the kernels of mppi_update.h / mppi_resident.h over them,
// k_fleet.hip the fleet forms of the batch prologue (mppi_fleet.h).  Everything here is __forceinline__: no unit exports it.
#pragma once
#include "fast_trig.h"
#include "mppi_device_util.h"
#include "mppi_resident.h"

namespace ccv {

// a value as two self-validating packets {32 data bits, 32-bit sequence number}, each one atomic store: the mailbox's and
// the exchange's format (mppi_update.h).  (seq by reference: read at each store, where the writers have always read it)
__device__ __forceinline__ void store_packets(unsigned long long* dst, const double value, const uint32_t& seq) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(value);
    __hip_atomic_store(dst + 0, (bits & 0xFFFFFFFF00000000ull) | seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 1, (bits << 32) | seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void mail_post(const FinalizeArgs& A, const int slot, const double value) {
    store_packets(A.mail + 2 * (size_t)slot, value, A.mail_seq);
}

// One wave per row n: lanes read the chunk partials of the row (fixed order => bitwise reproducible), wave-reduce them,
// and re-derive S = sum w the same way, so no cross-block hand-off is needed.  u*[n] = V_n / S
// (== sum_i (w_i/S) u_i of dd:222,234 up to rounding; S == 0 gives NaN exactly as dd:222 does).
// sums of two rows of n partials each (lane l takes columns l, l+64, ...): up to 1024 columns per pass, all 32 loads of a
// lane issued before the first add (one memory latency for both rows, not one per row)
__device__ __forceinline__ void lane_partial_sum2(const double* row_a, const double* row_b, int n, int lane, double& sum_a,
                                                  double& sum_b) {
    double acc_a = 0.0, acc_b = 0.0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        double va[16], vb[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = min(c0 + lane + 64 * i, n - 1);   // (clamped: the loads carry no branch)
            va[i] = row_a[c];
            vb[i] = row_b[c];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in = c0 + lane + 64 * i < n;
            acc_a += in ? va[i] : 0.0;
            acc_b += in ? vb[i] : 0.0;
        }
    }
    sum_a = acc_a;
    sum_b = acc_b;
}

// ---- batch handles, shifted weights (ccv_mppi_batch_set_min_shift) ------------------------------------------------------
// The SHIFT rollout kernels (pc_shifted_weight) leave, per workgroup g of 64 samples, sums of weights relative to the
// workgroup's own minimum cost m_g = statpart[g][0].  Relative to the instance's minimum m = min_g m_g the workgroup's sums
// carry the scale s_g = exp(-(m_g - m) / lambda): the best sample's weight and its workgroup's scale are exactly 1, so S >= 1.
// Sums of two rows of n scaled partials, columns and order as lane_partial_sum2.  Up to 1024 columns the three loads of a
// column (m_g, both rows) are all issued before the first compare: one memory latency for the minimum and the sums together;
// beyond, the minimum takes passes of its own first (all loads of a pass before its first compare) and the later columns
// are fetched again.  m_g = +inf (no finite cost in the workgroup): s_g = 0 against partials of 0; m = +inf: NaN.
__device__ __forceinline__ void shift_scaled_sum2(const double* row_a, const double* row_b, const double* statpart,
                                                  const double lambda, const int n, const int lane, double& sum_a,
                                                  double& sum_b) {
    double va[16], vb[16], mg[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = min(lane + 64 * i, n - 1);   // (clamped: the loads carry no branch)
        mg[i] = statpart[c * 3 + 0];
        va[i] = row_a[c];
        vb[i] = row_b[c];
    }
    double mn = INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) mn = fmin(mn, lane + 64 * i < n ? mg[i] : INFINITY);
    for (int c0 = 1024; c0 < n; c0 += 1024) {
        double a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = statpart[min(c0 + lane + 64 * i, n - 1) * 3 + 0];
#pragma unroll
        for (int i = 0; i < 16; ++i) mn = fmin(mn, c0 + lane + 64 * i < n ? a[i] : INFINITY);
    }
    const double m = wave_min(mn);
    double acc_a = 0.0, acc_b = 0.0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        if (c0 != 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = min(c0 + lane + 64 * i, n - 1);
                mg[i] = statpart[c * 3 + 0];
                va[i] = row_a[c];
                vb[i] = row_b[c];
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in = c0 + lane + 64 * i < n;
            const double sg = exp(-(mg[i] - m) / lambda);
            acc_a += in ? sg * va[i] : 0.0;
            acc_b += in ? sg * vb[i] : 0.0;
        }
    }
    sum_a = acc_a;
    sum_b = acc_b;
}

// what a statistics wave leaves (lane 0)
__device__ __forceinline__ void post_cost_stats(const FinalizeArgs& A, const int lane, const double mn, const double mx, const double nz) {
    if (lane == 0) {
        A.stats[1] = mn;
        A.stats[2] = mx;
        A.stats[3] = nz;
        if (A.mail) {
            mail_post(A, A.R + 1, mn);
            mail_post(A, A.R + 2, mx);
            mail_post(A, A.R + 3, nz);
        }
    }
}

// min / max cost and the zero-weight count over the per-workgroup statistics: a wave of its own (n == R + 1), so that its
// loads run beside the row reductions instead of after one of them
__device__ __forceinline__ void finalize_cost_stats(const FinalizeArgs& A, const int lane) {
    double mn = INFINITY, mx = -INFINITY, nz = 0.0;
    for (int c0 = 0; c0 < A.nchunks; c0 += 1024) {
        double a[16], b[16], z[16];
        #pragma unroll
        for (int i = 0; i < 16; ++i) {   // all loads first: one memory latency per 1024 partials
            const int c = min(c0 + lane + 64 * i, A.nchunks - 1);
            a[i] = A.statpart[c * 3 + 0];
            b[i] = A.statpart[c * 3 + 1];
            z[i] = A.statpart[c * 3 + 2];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in = c0 + lane + 64 * i < A.nchunks;
            mn = fmin(mn, in ? a[i] : INFINITY);
            mx = fmax(mx, in ? b[i] : -INFINITY);
            nz += in ? z[i] : 0.0;
        }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    nz = wave_sum(nz);
    post_cost_stats(A, lane, mn, mx, nz);
}
// the statistics wave in shifted-weight mode: min_cost = m, max_cost, and the zero-weight count -- the live samples whose
// block-relative weight is 0 in the workgroups whose scale is not 0 (statpart[g][2]), plus every live sample (64, or what is
// left of K in the last workgroup) of a workgroup whose scale is 0
__device__ __forceinline__ void finalize_cost_stats_shift(const FinalizeArgs& A, const double lambda, const int K, const int lane) {
    double mn = INFINITY;
    for (int c0 = 0; c0 < A.nchunks; c0 += 1024) {
        double a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = A.statpart[min(c0 + lane + 64 * i, A.nchunks - 1) * 3 + 0];
#pragma unroll
        for (int i = 0; i < 16; ++i) mn = fmin(mn, c0 + lane + 64 * i < A.nchunks ? a[i] : INFINITY);
    }
    const double m = wave_min(mn);
    double mx = -INFINITY, nz = 0.0;
    for (int c0 = 0; c0 < A.nchunks; c0 += 1024) {
        double a[16], b[16], z[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = min(c0 + lane + 64 * i, A.nchunks - 1);
            a[i] = A.statpart[c * 3 + 0];
            b[i] = A.statpart[c * 3 + 1];
            z[i] = A.statpart[c * 3 + 2];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = c0 + lane + 64 * i;
            const bool in = c < A.nchunks;
            const double sg = exp(-(a[i] - m) / lambda);
            const double all = (double)min(kPcSamples, K - c * kPcSamples);
            mx = fmax(mx, in ? b[i] : -INFINITY);
            nz += in ? (sg == 0.0 ? all : z[i]) : 0.0;
        }
    }
    mx = wave_max(mx);
    nz = wave_sum(nz);
    post_cost_stats(A, lane, m, mx, nz);
}

// The weight mode of an update: how a wave sums S = row R and one more row of the partials, and its statistics wave.
// (stride: the row pitch of the partials, nchunks but for a batch handle's fused partials; lambda, K: the instance's, SHIFT only)
template <bool SHIFT>
struct RowSum {
    double lambda = 0.0;
    int K = 0;
    __device__ __forceinline__ void operator()(const FinalizeArgs& A, const size_t stride, const int row, const int lane, double& s,
                                               double& v) const {
        const double* row_s = A.partial + (size_t)A.R * stride;
        const double* row_v = A.partial + (size_t)row * stride;
        if constexpr (SHIFT) shift_scaled_sum2(row_s, row_v, A.statpart, lambda, A.nchunks, lane, s, v);
        else lane_partial_sum2(row_s, row_v, A.nchunks, lane, s, v);
        s = wave_sum(s);
        v = wave_sum(v);
    }
    __device__ __forceinline__ void stats(const FinalizeArgs& A, const int lane) const {
        if constexpr (SHIFT) finalize_cost_stats_shift(A, lambda, K, lane);
        else finalize_cost_stats(A, lane);
    }
};

// what an update wave leaves: row n < R's V_n (and u*[n] = V_n / S), wave R's S
__device__ __forceinline__ void publish_row(const FinalizeArgs& A, const int n, const double s, const double v) {
    const int lane = threadIdx.x & 63;
    if (n < A.R && lane == 0) {
        A.vec[1 + n] = v;
        if (A.normalise) {
            const double q = v / s;
            A.nominal[n] = q;
            if (A.mail) mail_post(A, n, q);
        }
    }
    if (n == A.R && lane == 0) {
        A.vec[0] = s;
        A.stats[0] = s;
        if (A.mail) mail_post(A, A.R, s);
    }
}
template <class Sum>
__device__ __forceinline__ void finalize_rows(const FinalizeArgs& A, const size_t stride, const Sum& sum) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (n > A.R) {
        if (n == A.R + 1) sum.stats(A, lane);
        return;
    }
    double s, v;
    sum(A, stride, n < A.R ? n : A.R, lane, s, v);
    publish_row(A, n, s, v);
}

// ---- device-resident closed loop (mppi_resident.h) ------------------------------------------------------------------
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

// the command u*[0][d] = V_d / S, d < udim_of(model), by the waves of one workgroup: finalize_rows' sums of the same partials in the same
// order, so the bits its waves write into the warm start (the prologue cannot wait for them)
template <class Sum>
__device__ __forceinline__ void form_command(double* cmd, const FinalizeArgs& F, const size_t stride, const int model, const Sum& sum) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ud = udim_of(model);
    for (int d = wv; d < ud; d += kBlock / 64) {
        double s, v;
        sum(F, stride, d, lane, s, v);
        if (lane == 0) cmd[d] = v / s;
    }
}

// ---- batch handles: the same prologue for B instances, one workgroup each (BatchAdvanceArgs, mppi_resident.h) -----------
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

}  // namespace ccv

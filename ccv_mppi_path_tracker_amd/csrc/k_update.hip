// translation unit: the small kernels around the rollout (declared in mppi_update.h and mppi_resident.h, launched by the
// host units of the C ABI): weighted update, re-derivation of the controls from the stored normals, MIN_SHIFT
// re-weighting, the read-back helpers, and the prologue of the device-resident loop.  No entry point is a template: every
// kernel is defined here and nowhere else (the device functions they share are templates over the weight mode; those that
// k_fleet.hip instantiates as well are in mppi_update_device.h).
#include "mppi_top_weights.h"
#include "mppi_update_device.h"

namespace ccv {

// ---- re-derivation of the controls (MaterializeArgs, mppi_update.h) ---------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_materialize_controls(const MaterializeArgs A) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const int n = blockIdx.y;
    if (k >= A.K) return;
    const int d = n % A.udim;
    double v = (double)A.z[(size_t)n * A.pitch + k] * A.sigma + A.nominal_used[n];
    v = clampd(v, A.umin[d], A.umax[d]);
    if (d == A.zero_dim) v = 0.0;
    A.u[(size_t)n * A.pitch + k] = v;
}

// ---- weighted update -------------------------------------------------------------------------------------------
// grid (nchunks, R+1).  Row n < R: sum_k w_k*u[n][k] over this chunk; row R: sum_k w_k (+ cost stats).
// Fixed reduction order => bitwise reproducible (no atomics).
__device__ __forceinline__ void update_partials(const UpdateArgs& A) {
    __shared__ double red[4][4];
    const int row = blockIdx.y;
    const int chunk = blockIdx.x;
    const int base = chunk * kChunk;
    const bool wrow = row == A.R;
    const double* urow = A.u + (size_t)row * A.pitch;
    double acc = 0.0, mn = INFINITY, mx = -INFINITY, nz = 0.0;
#pragma unroll
    for (int i = 0; i < kChunk / (2 * kBlock); ++i) {
        const int k = base + i * 2 * kBlock + threadIdx.x * 2;
        if (k + 1 < A.K) {
            const double2 wv = *reinterpret_cast<const double2*>(A.w + k);
            if (wrow) {
                acc += wv.x;
                acc += wv.y;
                const double2 cv = *reinterpret_cast<const double2*>(A.cost + k);
                mn = fmin(mn, fmin(cv.x, cv.y));
                mx = fmax(mx, fmax(cv.x, cv.y));
                nz += (wv.x == 0.0 ? 1.0 : 0.0) + (wv.y == 0.0 ? 1.0 : 0.0);
            } else {
                const double2 uv = *reinterpret_cast<const double2*>(urow + k);
                acc += wv.x * uv.x;
                acc += wv.y * uv.y;
            }
        } else if (k < A.K) {
            const double wv = A.w[k];
            if (wrow) {
                acc += wv;
                const double cv = A.cost[k];
                mn = fmin(mn, cv);
                mx = fmax(mx, cv);
                nz += (wv == 0.0 ? 1.0 : 0.0);
            } else {
                acc += wv * urow[k];
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    acc = wave_sum(acc);
    if (wrow) {
        mn = wave_min(mn);
        mx = wave_max(mx);
        nz = wave_sum(nz);
    }
    if (lane == 0) {
        red[0][wid] = acc;
        red[1][wid] = mn;
        red[2][wid] = mx;
        red[3][wid] = nz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        A.partial[(size_t)row * A.nchunks + chunk] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        if (wrow) {
            A.statpart[chunk * 3 + 0] = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
            A.statpart[chunk * 3 + 1] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
            A.statpart[chunk * 3 + 2] = (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_update_partials(const UpdateArgs A) { update_partials(A); }
// Batch handles (the plain kernel's iteration): grid (nchunks, R+1, B).  Instance blockIdx.z owns the columns
// [z * kpad, z * kpad + K) of the shared rows and a block of partials [(R+1)][nchunks] and statistics [nchunks][3] of its own:
// the single handle's reduction, instance by instance.
__global__ __launch_bounds__(kBlock) void k_update_partials_batch(UpdateArgs A, const int kpad) {
    const size_t b = blockIdx.z;
    A.u += b * kpad;
    A.w += b * kpad;
    A.cost += b * kpad;
    A.partial += b * (size_t)(A.R + 1) * A.nchunks;
    A.statpart += b * (size_t)A.nchunks * 3;
    update_partials(A);
}

__global__ __launch_bounds__(kBlock) void k_finalize(const FinalizeArgs A) { finalize_rows(A, (size_t)A.nchunks, RowSum<false>{}); }

// grid (finalize_blocks(R), B); instance blockIdx.y reduces its own columns in the single handle's order (the same bits), every
// packet under the launch's one sequence number
__global__ __launch_bounds__(kBlock) void k_finalize_batch(FinalizeArgs A, const int fused) {
    const size_t b = blockIdx.y;
    const size_t stride = fused ? (size_t)gridDim.y * A.nchunks : (size_t)A.nchunks;
    A.partial += fused ? b * A.nchunks : b * (size_t)(A.R + 1) * A.nchunks;
    A.statpart += b * (size_t)A.nchunks * 3;
    A.nominal += b * A.R;
    A.vec += b * (size_t)(A.R + 1);
    A.stats += b * 4;
    if (A.mail) A.mail += 2 * b * (size_t)(A.R + 4);
    finalize_rows(A, stride, RowSum<false>{});
}
// k_finalize_batch over the SHIFT rollout kernels' partials (always the fused layout): grid (finalize_blocks(R), B);
// P: the parameter table (instance y's lambda), K: samples per instance
__global__ __launch_bounds__(kBlock) void k_finalize_batch_shift(FinalizeArgs A, const BatchParams* P, const int K) {
    const size_t b = blockIdx.y;
    const size_t stride = (size_t)gridDim.y * A.nchunks;
    A.partial += b * A.nchunks;
    A.statpart += b * (size_t)A.nchunks * 3;
    A.nominal += b * A.R;
    A.vec += b * (size_t)(A.R + 1);
    A.stats += b * 4;
    if (A.mail) A.mail += 2 * b * (size_t)(A.R + 4);
    finalize_rows(A, stride, RowSum<true>{P[b].lambda, K});
}

// ---- direct exchange (ExchangeBox, ExchangeArgs: mppi_update.h) ---------------------------------------------------------
__device__ __forceinline__ unsigned long long load_system(const unsigned long long* p) {   // past every cache
    unsigned long long v;
    asm volatile("global_load_dwordx2 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    return v;
}

__global__ __launch_bounds__(kBlock) void k_finalize_exchange(const FinalizeArgs A, const ExchangeArgs X) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   // rows 0..R-1; wave R: sum w; wave R + 1: cost statistics
    if (n > A.R) {
        if (n == A.R + 1) finalize_cost_stats(A, lane);   // (this device's samples only)
        return;
    }
    double s, v;
    RowSum<false>{}(A, (size_t)A.nchunks, n < A.R ? n : A.R, lane, s, v);
    // ---- this wave's value into slot [rank] of every peer's box: lane d writes to rank d
    const int slot = n < A.R ? 1 + n : 0;
    const double mine = n < A.R ? v : s;
    if (lane < X.world) {
        const uint32_t seq = X.seq;
        store_packets(&X.peer[lane]->pkt[X.parity][X.rank][slot][0], mine, seq);
    }
    if (lane == 0) {   // (this device's share)
        A.vec[slot] = mine;
        if (n == A.R) A.stats[0] = s;
    }
    // ---- the peers' values of the same slot: lane r polls rank r's two packets in the local box
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long* src = &X.local->pkt[X.parity][lane < X.world ? lane : 0][slot][0];
    unsigned long long hi = 0, lo = 0;
    bool arrived = lane >= X.world;
    while (true) {
        if (!arrived) {
            hi = load_system(src + 0);
            lo = load_system(src + 1);
            arrived = (uint32_t)hi == X.seq && (uint32_t)lo == X.seq;
        }
        if (__all(arrived)) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > X.timeout_ticks) break;
        __builtin_amdgcn_s_sleep(4);
    }
    const bool ok = __all(arrived);
    const double theirs = __longlong_as_double((long long)((hi & 0xFFFFFFFF00000000ull) | (lo >> 32)));
    double acc = 0.0;
    for (int r = 0; r < X.world; ++r) acc += lane_value(theirs, r);   // rank order on every device
    if (lane == 0) {
        X.reduced[slot] = ok ? acc : __builtin_nan("");
        if (!ok && X.timeout_flag) __hip_atomic_store(X.timeout_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (pinned host memory)
    }
}

// After the cross-device all-reduce of [sum w, sum w*u]: u* = V / S on every device.
__global__ __launch_bounds__(kBlock) void k_apply_partials(const double* vec, double* nominal, double* stats, int R) {
    const double S = vec[0];
    if (threadIdx.x == 0) stats[0] = S;
    for (int n = threadIdx.x; n < R; n += kBlock) nominal[n] = vec[1 + n] / S;
}

// ---- optional underflow-safe weights (CCV_MPPI_FLAG_MIN_SHIFT; not reference behaviour) --------------------------
// the minimum of cost[0 .. K): one workgroup of 1024, the result in thread 0
__device__ __forceinline__ double block_min_cost(const double* cost, const int K) {
    __shared__ double red[16];
    double mn = INFINITY;
    for (int k = threadIdx.x; k < K; k += 1024) mn = fmin(mn, cost[k]);
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    double r = red[0];
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) r = fmin(r, red[i]);
    }
    return r;
}
__global__ __launch_bounds__(1024) void k_min_cost(const double* cost, int K, double* out_min) {
    const double r = block_min_cost(cost, K);
    if (threadIdx.x == 0) *out_min = r;
}
__global__ __launch_bounds__(kBlock) void k_reweight(const double* cost, const double* cmin, double lambda, int K, double* w) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < K) w[k] = exp(-(cost[k] - *cmin) / lambda);
}

// batch handles in shifted-weight mode, plain family: the exact minimum of every instance (grid B) and its weights re-formed
// around it with the instance's own lambda (grid (ceil(K / kBlock), B)), in front of k_update_partials_batch -- the single
// handle's MIN_SHIFT arithmetic, instance by instance
__global__ __launch_bounds__(1024) void k_min_cost_batch(const double* cost, int K, int kpad, double* out_min) {
    const double r = block_min_cost(cost + (size_t)blockIdx.x * kpad, K);
    if (threadIdx.x == 0) out_min[blockIdx.x] = r;
}
__global__ __launch_bounds__(kBlock) void k_reweight_batch(const double* cost, const double* cmin, const BatchParams* P, int K,
                                                          int kpad, double* w) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    const size_t b = blockIdx.y;
    if (k < K) w[b * kpad + k] = exp(-(cost[b * kpad + k] - cmin[b]) / P[b].lambda);
}

// ---- read-back helpers -----------------------------------------------------------------------------------------
// out[c][t][2] = (xs[t][first + c*stride], ys[t][...])
__global__ __launch_bounds__(kBlock) void k_gather_xy(const double* xs, const double* ys, int pitch, int H, int first,
                                                      int count, int stride, double* out) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count * H) return;
    const int c = idx / H, t = idx % H;
    const size_t src = (size_t)t * pitch + first + (size_t)c * stride;
    out[(size_t)idx * 2 + 0] = xs[src];
    out[(size_t)idx * 2 + 1] = ys[src];
}

// ---- top-N candidates by weight (publish_CandidatePath() feed, dd:265-294: at K = 65 536 rviz can only draw a few) ----
// One workgroup runs top_weights() of mppi_top_weights.h (the selection and its order are specified there); the host sorts the
// N pairs.
__global__ __launch_bounds__(kTopBlock) void k_top_weights(const double* w, int K, int N, int* idx_out, double* w_out) {
    top_weights<kTopBlock>(w, K, N, idx_out, w_out);
}

// gather of listed samples: out[c][t] = (x, y) of sample idx[c] at step t
__global__ __launch_bounds__(kBlock) void k_gather_xy_list(const double* xs, const double* ys, int pitch, int H, const int* idx,
                                                           int count, double* out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count * H) return;
    const int c = j / H, t = j % H;
    const size_t src = (size_t)t * pitch + idx[c];
    out[(size_t)j * 2 + 0] = xs[src];
    out[(size_t)j * 2 + 1] = ys[src];
}

__global__ __launch_bounds__(kBlock) void k_normalise_weights(const double* w, const double* stats, int first, int count,
                                                             double* out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) out[i] = w[first + i] / stats[0];
}

// shifted-weight mode of a batch handle (fused kernels): w holds block-relative weights; the normalised weight of sample k of
// workgroup g = k / 64 is w[k] * s_g / S with s_g as in shift_scaled_sum2 (statpart, stats: the instance's; stats[1] = m)
__global__ __launch_bounds__(kBlock) void k_normalise_weights_shift(const double* w, const double* statpart, const double* stats,
                                                                   double lambda, int first, int count, double* out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int k = first + i;
    const double sg = exp(-(statpart[(k / kPcSamples) * 3 + 0] - stats[1]) / lambda);
    out[i] = (w[k] * sg) / stats[0];
}

// ---- device-resident closed loop (mppi_resident.h; advance_body: mppi_update_device.h) ----------------------------------
__global__ __launch_bounds__(kAdvanceThreads) void k_advance(const AdvanceArgs A) { advance_body<kAdvanceThreads>(A, A.nominal); }

// The update of tick i and the prologue of tick i+1 in ONE launch (the closed loop then costs two launches per tick, not
// three): blocks 0 .. finalize_blocks(R)-1 are k_finalize; one more block forms the command and runs the prologue with it.
__global__ __launch_bounds__(kBlock) void k_finalize_advance(const FinalizeArgs F, const AdvanceArgs A) {
    if ((int)blockIdx.x < finalize_blocks(F.R)) {
        finalize_rows(F, (size_t)F.nchunks, RowSum<false>{});
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (A.advance) form_command(cmd, F, (size_t)F.nchunks, A.model, RowSum<false>{});
    __syncthreads();
    advance_body<kBlock>(A, cmd);
}

// ---- batch handles: the same prologue for B instances, one workgroup each (BatchAdvanceArgs, mppi_resident.h) -----------
// grid B: instance blockIdx.x, its command read from u*[b][0]
__global__ __launch_bounds__(kBatchAdvanceThreads) void k_advance_batch(const BatchAdvanceArgs G) {
    double* rec;
    const AdvanceArgs A = batch_advance_view(G, (int)blockIdx.x, rec);
    advance_body<kBatchAdvanceThreads, true>(A, A.nominal, rec);
}

// The batched k_finalize_advance: grid (finalize_blocks(R) + 1, B).  Blocks x < finalize_blocks(R) are k_finalize_batch
// (fused partials) for instance y; block x = finalize_blocks(R) forms instance y's command from
// the instance's own partial columns and runs the instance's prologue with it.
template <bool VARIED>
__device__ __forceinline__ void finalize_advance_batch(FinalizeArgs I, const BatchAdvanceArgs& G, const BatchParams* P) {
    const size_t b = blockIdx.y;
    const size_t stride = (size_t)gridDim.y * I.nchunks;
    const RowSum<false> sum{};
    I.partial += b * I.nchunks;
    if ((int)blockIdx.x < finalize_blocks(I.R)) {
        I.statpart += b * (size_t)I.nchunks * 3;
        I.nominal += b * I.R;
        I.vec += b * (size_t)(I.R + 1);
        I.stats += b * 4;
        finalize_rows(I, stride, sum);   // (no mailbox: a deferred update is never a blocking call's)
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (G.advance) form_command(cmd, I, stride, G.model, sum);
    __syncthreads();
    double* rec;
    const AdvanceArgs A = batch_advance_view<VARIED>(G, (int)b, rec, P);
    advance_body<kBlock, true>(A, cmd, rec);
}
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch(FinalizeArgs F, const BatchAdvanceArgs G) {
    finalize_advance_batch<false>(F, G, nullptr);
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

// ... over the SHIFT rollout kernels' partials: the update blocks are k_finalize_batch_shift's, and the extra block forms the
// command with shift_scaled_sum2 as well.  (A body and a command loop of its own: through finalize_advance_batch and
// form_command the compiler lays the same instructions out in another order.)
__global__ __launch_bounds__(kBlock) void k_finalize_advance_batch_shift(FinalizeArgs F, const BatchAdvanceArgs G, const BatchParams* P) {
    const size_t b = blockIdx.y;
    const size_t stride = (size_t)gridDim.y * F.nchunks;
    const double lambda = P[b].lambda;
    F.partial += b * F.nchunks;
    F.statpart += b * (size_t)F.nchunks * 3;
    if ((int)blockIdx.x < finalize_blocks(F.R)) {
        F.nominal += b * F.R;
        F.vec += b * (size_t)(F.R + 1);
        F.stats += b * 4;
        finalize_rows(F, stride, RowSum<true>{lambda, G.K});   // (no mailbox: a deferred update is never a blocking call's)
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (G.advance) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ud = udim_of(G.model);
        for (int d = wv; d < ud; d += kBlock / 64) {
            double s, v;
            shift_scaled_sum2(F.partial + (size_t)F.R * stride, F.partial + (size_t)d * stride, F.statpart, lambda, F.nchunks, lane, s, v);
            s = wave_sum(s);
            v = wave_sum(v);
            if (lane == 0) cmd[d] = v / s;
        }
    }
    __syncthreads();
    double* rec;
    const AdvanceArgs A = batch_advance_view<true>(G, (int)b, rec, P);
    advance_body<kBlock, true>(A, cmd, rec);
}

}  // namespace ccv

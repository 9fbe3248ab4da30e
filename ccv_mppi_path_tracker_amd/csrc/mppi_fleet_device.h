// The device functions of the fleet forms of the batch prologue kernels (mppi_fleet.h; DESIGN.md sections 10f, 10g): the fleet step
// and the publication of a robot's new position, shared by k_fleet.hip and, with PRED, k_fleet_pred.hip.  Everything PRED adds is
// compiled out when it is false.
#pragma once
#include "mppi_fleet.h"
#include "mppi_update_device.h"

namespace ccv {

// Instance y's neighbour discs for this tick, by the kBlock threads of its prologue workgroup (spec: DESIGN.md section 10f;
// the library is built with -ffp-contract=off and nothing here is an FMA, so numpy reproduces every bit).
//   d2_j = dx*dx + dy*dy with dx = q_j[0] - q_y[0], dy = q_j[1] - q_y[1]; j != y is a candidate iff d2_j <= range2 (a NaN
//   fails); the candidates in (d2, j) order, the first M_y = min(max_neighbours, 32 - n_static[y]) of them become rows
//   (q_j[0], q_j[1], radius[y] + radius[j]) n_static[y] .. of the instance's list, and n_obst = n_static[y] + their number.
// A candidate's row index is its rank, the number of candidates before it in that order, counted in a loop over LDS: no
// atomics and no sort.  The workgroup's width is fixed: thread t holds robots t, t + kBlock, ... in kPer = kFleetMaxBatch / kBlock
// registers, so every robot has a thread only when the workgroup has exactly kBlock threads -- which the fused forms have by
// their launch and the prologue kernels of their own because kBatchAdvanceThreads == kBlock (asserted beside kPer).  Which
// thread or wave holds a robot changes no result: ties go by j, and the count is the sum of all kBlock / 64 wave totals.  The
// LDS first holds the positions, then the keys: d2_j for a candidate, NaN otherwise (a NaN key is before nothing and after
// nothing).
// PRED (fleet prediction): a selected neighbour's velocity, formed by that robot's own prologue block one
// tick ago (fleet_publish), goes into the velocity row that belongs to the disc row; the selection itself does not change.
template <bool PRED = false>
__device__ __forceinline__ void fleet_step(const FleetArgs& L, BatchParams* P, const int y, const FleetPredArgs* V = nullptr) {
    constexpr int kPer = kFleetMaxBatch / kBlock;   // candidates per thread: j = threadIdx.x + i * kBlock
    static_assert(kPer * kBlock == kFleetMaxBatch && kBatchAdvanceThreads == kBlock && kBlock % 64 == 0,
                  "fleet_step: kBlock threads, whichever kernel it is in, cover kFleetMaxBatch robots in kPer strides");
    __shared__ double s_key[2 * kFleetMaxBatch];    // [B][2] positions; then [B] keys
    __shared__ int s_cnt[kBlock / 64];
    const int B = L.B < kFleetMaxBatch ? L.B : kFleetMaxBatch;   // (the host refuses larger batches)
    for (int j = threadIdx.x; j < B; j += kBlock) {
        const double2 q = reinterpret_cast<const double2*>(L.xy_in)[j];
        s_key[2 * j] = q.x;
        s_key[2 * j + 1] = q.y;
    }
    __syncthreads();
    const double qx = s_key[2 * y], qy = s_key[2 * y + 1];
    double px[kPer], py[kPer], d2[kPer];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int j = threadIdx.x + i * kBlock;
        px[i] = py[i] = 0.0;
        d2[i] = __builtin_nan("");
        if (j < B) {
            px[i] = s_key[2 * j];
            py[i] = s_key[2 * j + 1];
            const double dx = px[i] - qx, dy = py[i] - qy;
            const double d = dx * dx + dy * dy;
            if (j != y && d <= L.range2) {
                d2[i] = d;
                mine += 1;
            }
        }
    }
    __syncthreads();   // (every thread has read its positions)
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int j = threadIdx.x + i * kBlock;
        if (j < B) s_key[j] = d2[i];
    }
    // the number of candidates: wave sums (DPP), then the kBlock / 64 wave totals through LDS
    const double wave_total = wave_sum((double)mine);   // (exact: at most 64 * kPer)
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (int)wave_total;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) total += s_cnt[w];
    const int ns_raw = L.n_static[y];
    const int ns = ns_raw < 0 ? 0 : (ns_raw > kMaxObst ? kMaxObst : ns_raw);
    const int room = kMaxObst - ns;
    const int M = L.max_neighbours < room ? (L.max_neighbours < 0 ? 0 : L.max_neighbours) : room;
    const double ry = L.radius[y];
    double* rows = L.obst + ((size_t)y * kMaxObst + ns) * 3;
    double* vrows = nullptr;
    if constexpr (PRED) vrows = V->obst_v + ((size_t)y * kMaxObst + ns) * 2;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int j = threadIdx.x + i * kBlock;
        const double d = d2[i];
        if (!(d == d) || M == 0) continue;   // (not a candidate)
        int rank = 0;
        for (int k = 0; k < B; ++k) {
            const double o = s_key[k];
            rank += (o < d || (o == d && k < j)) ? 1 : 0;
        }
        if (rank < M) {   // (rank < M <= 32 - ns: inside the instance's 32 rows)
            rows[3 * rank + 0] = px[i];
            rows[3 * rank + 1] = py[i];
            rows[3 * rank + 2] = ry + L.radius[j];
            if constexpr (PRED) {
                const double2 v = reinterpret_cast<const double2*>(V->v_in)[j];
                vrows[2 * rank + 0] = v.x;
                vrows[2 * rank + 1] = v.y;
            }
        }
    }
    if (threadIdx.x == 0) P[y].n_obst = ns + (total < M ? total : M);
    __syncthreads();   // (advance_body's LDS follows)
}

// instance y's position after this tick's advance, for the next tick's snapshot: thread 0 of the prologue workgroup wrote the
// frame's pose (advance_body) and reads its own stores back
// PRED: and its velocity over this tick, v = (after - before) * inv_dt -- one fp64 subtraction and one multiplication per
// component, no FMA, with the inv_dt the step carries; before = its position in this tick's snapshot.  Zero when the tick does
// not advance, when dt = 0, or when a component is not finite.
template <bool PRED = false>
__device__ __forceinline__ void fleet_publish(const FleetArgs& L, const ResidentFrame* frames, const int y, const BatchAdvanceArgs* G = nullptr,
                                              const FleetPredArgs* V = nullptr) {
    if (threadIdx.x == 0) {
        const double x = frames[y].x0[0], yy = frames[y].x0[1];
        reinterpret_cast<double2*>(L.xy_out)[y] = make_double2(x, yy);
        if constexpr (PRED) {
            const double2 q = reinterpret_cast<const double2*>(L.xy_in)[y];
            double vx = (x - q.x) * G->inv_dt, vy = (yy - q.y) * G->inv_dt;
            const bool ok = G->advance && G->dt != 0.0 && isfinite(vx) && isfinite(vy);
            if (!ok) vx = vy = 0.0;
            reinterpret_cast<double2*>(V->v_out)[y] = make_double2(vx, vy);
        }
    }
}

// the two fused forms, written once: grid (finalize_blocks(R) + 1, B).  The update blocks are k_finalize_batch's (SHIFT:
// k_finalize_batch_shift's); the extra block of instance b forms the command with the same row sum, runs the fleet step and
// the prologue, and publishes the new position
template <bool SHIFT, bool PRED = false>
__device__ __forceinline__ void finalize_advance_fleet(FinalizeArgs& F, const BatchAdvanceArgs& G, BatchParams* P, const FleetArgs& L,
                                                       const RowSum<SHIFT>& sum, const FleetPredArgs* V = nullptr) {
    const size_t b = blockIdx.y;
    const size_t stride = (size_t)gridDim.y * F.nchunks;
    F.partial += b * F.nchunks;
    if constexpr (SHIFT) F.statpart += b * (size_t)F.nchunks * 3;   // (the shifted row sum of the extra block reads it too)
    if ((int)blockIdx.x < finalize_blocks(F.R)) {
        if constexpr (!SHIFT) F.statpart += b * (size_t)F.nchunks * 3;
        F.nominal += b * F.R;
        F.vec += b * (size_t)(F.R + 1);
        F.stats += b * 4;
        finalize_rows(F, stride, sum);   // (no mailbox: a deferred update is never a blocking call's)
        return;
    }
    __shared__ double cmd[CCV_MPPI_MAX_UDIM + 3];
    if (G.advance) form_command(cmd, F, stride, G.model, sum);
    fleet_step<PRED>(L, P, (int)b, V);   // (ends in a barrier: cmd is complete behind it)
    double* rec;
    const AdvanceArgs A = batch_advance_view<true>(G, (int)b, rec, P);
    advance_body<kBlock, true>(A, cmd, rec);
    fleet_publish<PRED>(L, G.frames, (int)b, &G, V);
}

}  // namespace ccv

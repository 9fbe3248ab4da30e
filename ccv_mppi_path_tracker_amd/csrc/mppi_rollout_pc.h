// k_rollout_pc: the two-wave sample + rollout + cost kernel ("producer / consumer" time blocks) -- the production kernel
// of the full-body model -- over the building blocks it shares with the other cooperative families (mppi_produce.h,
// mppi_consume.h, mppi_epilogue.h, mppi_handoff.h).
//
// One sample per lane.  A workgroup is TWO waves that own the same 64 samples and alternate roles over time blocks
// of kTU = 8 steps:
//
//   step s:   wave (s & 1)        PRODUCES block s   : Philox noise -> clamped controls -> HBM, Euler rollout with sincos,
//                                                      x,y -> HBM, control / ZMP cost terms; hands (x,y) of its 8 states
//                                                      and the end state to the other wave through LDS
//             wave ((s - 1) & 1)  CONSUMES block s-1 : squared distance of its 8 states to every point of the reference
//                                                      window (2 FMA + 1 MIN per pair, the O(K*H^2) core) -> path cost
//             barrier
//
// Why: at K = 65 536 a plain one-sample-per-lane grid is exactly one wave per SIMD (1024 waves on 1024 SIMDs) and
// every stall is exposed -- the wave that waits for a store slot, an LDS broadcast or a Philox multiply leaves its
// SIMD idle (measured 75 us for one iteration vs 41 us per 65 536 samples once 8 waves share a SIMD).  Splitting the
// sample's work by time block gives 2048 waves (2 per SIMD) with complementary instruction mixes (integer/trig/stores
// vs straight fp64 FMA/MIN) and no duplicated arithmetic: per sample the operations are exactly those of
// k_rollout_cost; only the order in which one sample's cost terms are added differs.
#pragma once
#include "mppi_consume.h"
#include "mppi_epilogue.h"
#include "mppi_handoff.h"
#include "mppi_produce.h"

namespace ccv {

constexpr int kPcWaves = 2;
template <int MODEL>
constexpr int kPcStateWords = MODEL == CCV_MPPI_FULL_BODY ? 12 : (MODEL == CCV_MPPI_DIFF_DRIVE ? 5 : 3);

template <int MODEL>
struct PcShared {
    // kStage: the producer hands its normals (sh.zs) and states to a store wave through LDS instead of storing them itself
    // (mppi_rollout_r3.h, mppi_rollout_r4.h); here it stores them to HBM directly
    static constexpr bool kStage = false;
    static constexpr int kPBuf = 2;              // buffers of p: the block being produced and the one being consumed
    double2 ab[kMaxH + 4];                                 // window coefficients, padded to a multiple of 4 points
    double c[kMaxH + 4];
    double p[2][kTU][2][kPcSamples];                       // (x,y) - pose of the 8 states of a block, double buffered
    // producer -> next producer.  One buffer is enough: the producer of block s reads it first thing and writes it last,
    // the other wave reads it only after the barrier that ends the step
    double st[kPcStateWords<MODEL>][kPcSamples];
    double cost[kPcWaves][kPcSamples];
    alignas(32) double nom[(kMaxH + 8) * udim_of(MODEL)];  // warm start u* (see pc_stage_nominal)
    // full body: normals made ahead by each wave for the block it produces next (pc_noise_ahead)
    float ahead[MODEL == CCV_MPPI_FULL_BODY ? kPcWaves : 1][MODEL == CCV_MPPI_FULL_BODY ? 16 : 1][kPcSamples];
};

// this kernel's row dealing (UpdRowsT, mppi_epilogue.h): units of one time block's rows, two waves
template <int MODEL>
using UpdRows = UpdRowsT<kTU * udim_of(MODEL), kPcWaves>;

template <int MODEL, class T>
__device__ __forceinline__ void pc_partial_update(const RolloutArgs& A, PcShared<MODEL>& sh, T (&v)[kUpdCH],
                                                  const UpdRows<MODEL>& rows, const int mcount, const double wgt,
                                                  const double total, const int lane, const int wv, const int kk,
                                                  const bool live) {
    // sh.p: 8 * 2 * 64 = 1024 doubles per wave, free after the last consume (the caller has passed the barrier)
    pc_reduce_rows<kUpdRB, MODEL>(A, sh, &sh.p[wv][0][0][0], v, rows, mcount, wgt, lane, kk);
    if (wv == 0) pc_block_stats(A, (A.H - 1) * udim_of(MODEL), wgt, total, live, lane);
}

template <int MODEL, int MODE>
__global__ __launch_bounds__(kPcWaves * 64, 2) void k_rollout_pc(const RolloutArgs Ak, const Window Wk) {
    constexpr bool FB = MODEL == CCV_MPPI_FULL_BODY;
    constexpr bool COST = MODE != MODE_ROLLOUT;
    __shared__ PcShared<MODEL> sh;
    const RolloutArgs A = with_resident_pose(Ak);
    const int H = A.H;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (COST) stage_window(A, Wk, sh, kPcWaves * 64);
    if constexpr (MODE == MODE_FUSED) pc_stage_nominal<MODEL>(A, sh, kPcWaves * 64);
    const int k = blockIdx.x * kPcSamples + lane;
    const bool live = k < A.K;
    const int kk = live ? k : A.K - 1;
    const uint32_t kg = (uint32_t)(A.k_offset + kk);
    double cost = 0.0;
    if (wv == 0) cost += pc_initial_cost<MODEL, MODE>(A);
    const int nblocks = (H + kTU - 1) / kTU;
    const int nstates = FB ? H - 2 : H;   // states that reach the path cost (dd:199 / fb:409)
    int prune_on = 1;
    constexpr bool AHEAD = FB && MODE == MODE_FUSED;   // pc_noise_ahead
    __syncthreads();
    for (int s = 0; s <= nblocks; ++s) {
        pc_rotate_priority(A, s);
        if (s < nblocks && (s & 1) == wv) {
            // ---------------- produce block s
            PcState<MODEL> S;
            if (s == 0) {
                pc_initial_state<MODEL>(A, S);
            } else {
                const double(*st)[kPcSamples] = sh.st;
                S.x = st[0][lane];
                S.y = st[1][lane];
                S.yaw = st[2][lane];
                if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
                    S.sn = st[3][lane];
                    S.cs = st[4][lane];
                }
                if constexpr (FB) {
                    S.roll = st[3][lane];
                    S.pitch = st[4][lane];
                    S.p_v = st[5][lane];
                    S.p_rv = st[6][lane];
                    S.p_sdir = st[7][lane];
                    S.p_cdir = st[8][lane];
                    S.p_c2 = st[9][lane];
                    S.p_c3 = st[10][lane];
                    S.p_ac = st[11][lane];
                }
            }
            const int nctl = min(kTU, H - 1 - s * kTU);   // steps of this block that carry controls
            const float(*ahead)[kPcSamples] = (AHEAD && s >= 1) ? sh.ahead[wv] : nullptr;
            if (nctl == kTU) pc_produce_batched<MODEL, MODE>(A, sh, S, cost, s, lane, k, kk, live, kg, ahead);
            else if (nctl >= kPartialMin) pc_produce_batched<MODEL, MODE, PcShared<MODEL>, kPartialBlock>(A, sh, S, cost, s, lane, k, kk, live, kg, ahead, nctl);
            else pc_produce<MODEL, MODE, false>(A, sh, S, cost, s, lane, k, kk, live, kg);   // (a short tail, or the final state only)
            double(*st)[kPcSamples] = sh.st;
            st[0][lane] = S.x;
            st[1][lane] = S.y;
            st[2][lane] = S.yaw;
            if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE) {
                st[3][lane] = S.sn;
                st[4][lane] = S.cs;
            }
            if constexpr (FB) {
                st[3][lane] = S.roll;
                st[4][lane] = S.pitch;
                st[5][lane] = S.p_v;
                st[6][lane] = S.p_rv;
                st[7][lane] = S.p_sdir;
                st[8][lane] = S.p_cdir;
                st[9][lane] = S.p_c2;
                st[10][lane] = S.p_c3;
                st[11][lane] = S.p_ac;
            }
        }
        if constexpr (COST) {
            if (s >= 1 && ((s - 1) & 1) == wv) {
                // ---------------- consume block s-1
                const int b = s - 1;
                const int nv = min(kTU, nstates - b * kTU);
                // (not pc_consume_states: with it, behind the nv == kTU branch or without, every instantiation that forms a cost
                //  compiled to other instructions)
                if (nv == kTU) pc_consume<kTU, MODEL>(A, sh, cost, b, lane, &prune_on);
                else if (nv > 0) {
                    switch (nv) {
                        case 7: pc_consume<7, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        case 6: pc_consume<6, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        case 5: pc_consume<5, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        case 4: pc_consume<4, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        case 3: pc_consume<3, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        case 2: pc_consume<2, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                        default: pc_consume<1, MODEL>(A, sh, cost, b, lane, &prune_on); break;
                    }
                }
            }
        }
        if constexpr (AHEAD) {
            // the wave that is not producing now produces block s+1 next: part of that block's normals, made in its idle time
            if (((s + 1) & 1) == wv && s + 1 < nblocks && H - 1 - (s + 1) * kTU >= kPartialMin)   // (a block made as a batch, full or partial)
                pc_noise_ahead<MODEL>(A, sh.ahead[wv], s + 1, lane, kg);
        }
        pc_barrier_lds();
    }
    if (A.prio_rotate) __builtin_amdgcn_s_setprio(0);
    if constexpr (COST) {
        UpdT<MODE> upd[kUpdCH];
        const UpdRows<MODEL> rows{(H - 1) * udim_of(MODEL), wv};
        const int mcount = A.fuse_update ? rows.count() : 0;
        // start the re-read of this wave's controls before anything else (see pc_update_fetch)
        if (mcount > 0) pc_update_fetch(A, upd, rows, 0, mcount, kk);
        sh.cost[wv][lane] = cost;
        pc_barrier_lds();   // also: everyone is done with sh.p
        const double total = sh.cost[0][lane] + sh.cost[1][lane];
        const double wgt = pc_weight<false>(A, total, live);
        if (wv == 0 && live) {
            A.cost[k] = total;
            A.w[k] = wgt;
        }
        if (A.fuse_update) pc_partial_update<MODEL>(A, sh, upd, rows, mcount, wgt, total, lane, wv, kk, live);
    }
}

}  // namespace ccv

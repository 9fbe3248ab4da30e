// One wave per 64 samples, everything in that wave: k_rollout_solo.
//
// The two- and three-wave kernels (mppi_rollout_pc.h, mppi_rollout_r3.h) split the work of 64 samples over several waves
// because at K = 65 536 there is only one block of 64 samples per SIMD, and a lone wave leaves the SIMD idle in every
// dependent chain.  Their price is the hand-off: a barrier per block of 8 time steps, and the waves of a workgroup wait for
// each other whenever a neighbour on their SIMD delays one of them (full body, K = 131 072: 29 % of the wave cycles are
// barrier waits).  Once K provides two or more blocks of 64 samples per SIMD the SIMD is kept busy by independent waves
// anyway, and the hand-off is pure loss: this kernel runs the same building blocks -- the batched branch-free producer
// (pc_produce_batched, mppi_produce.h), the software-pipelined distance loop (pc_consume, mppi_consume.h), the fused update
// epilogue (mppi_epilogue.h) -- in ONE wave per 64
// samples, producer and distance phase alternating in program order, the state in registers, no barrier in the time loop.
// The full-body model is the one that profits (its 230 VGPRs allow two waves per SIMD whatever the kernel shape).
#pragma once
#include "mppi_consume.h"
#include "mppi_epilogue.h"
#include "mppi_handoff.h"
#include "mppi_produce.h"

namespace ccv {

template <int MODEL>
struct SoloShared {
    static constexpr bool kStage = false;
    static constexpr int kPBuf = 1;                        // produced and consumed by the same wave, one after the other
    double2 ab[kMaxH + 4];                                 // window coefficients, padded to a multiple of 4 points
    double c[kMaxH + 4];
    double p[1][kTU][2][kPcSamples];                       // (x,y) - pose of the 8 states of a block; epilogue: transpose buffer
    alignas(32) double nom[(kMaxH + 8) * udim_of(MODEL)];  // warm start u*
};

// WIDE: see pc_produce_batched (diff drive beyond |w|max dt = pi/4); BATCH: a batch handle's launch (batch_view, mppi_kernels.h);
// VARIED: with the batch's per-instance parameters; SHIFT (on VARIED): block-relative weights (pc_shifted_weight);
// OBST (on VARIED): the instance's disc obstacles (obst_stage, obst_term); MOVING (on OBST): the discs move (obst_stage_moving,
// obst_term_moving); GRID (on MOVING): the instance's occupancy grid (grid_tap, mppi_cost_terms.h), looked up by the producer where
// it stores the block's absolute states; the block's gathers are summed after its distance phase, under which their latency
// passes.  The grid term is the last added to the cost.  Diff drive and steering only.
// FORM (BatchForm, mppi_kernels.h) names the rung; BATCH .. GRID below are "FORM is at least that rung".
template <int MODEL, int MODE, bool WIDE = false, BatchForm FORM = BatchForm::Single, bool SHIFT = false>
__global__ __launch_bounds__(kPcSamples, 2) void k_rollout_solo(const RolloutArgs Ak, const Window Wk) {
    constexpr bool BATCH = FORM >= BatchForm::Batch, VARIED = FORM >= BatchForm::Varied, OBST = FORM >= BatchForm::Obst,
                   MOVING = FORM >= BatchForm::Moving, GRID = FORM >= BatchForm::Grid;
    static_assert(MODE == MODE_FUSED, "the stage-wise modes use k_rollout_pc");
    static_assert(!SHIFT || VARIED, "the shifted weights are built on the per-instance-parameter kernels");
    // (the MOVING parent uses all 256 registers without a spill; with the term it spilled two or three whether the sum was held
    //  in registers or in LDS -- DESIGN.md section 10h -- so full-body grid plans run the four-wave form, make_plan)
    static_assert(!GRID || MODEL != CCV_MPPI_FULL_BODY, "the one-wave full-body kernel has no grid form");
    constexpr bool FB = MODEL == CCV_MPPI_FULL_BODY;
    __shared__ SoloShared<MODEL> sh;
    ObstLds* obst_lds = nullptr;   // (an array of its own: SoloShared stays as it is)
    ObstMovLds* obst_mov = nullptr;
    if constexpr (MOVING) {
        __shared__ ObstMovLds s_obst_mov;
        obst_mov = &s_obst_mov;
    } else if constexpr (OBST) {
        __shared__ ObstLds s_obst;
        obst_lds = &s_obst;
    }
    static_assert(sizeof(sh.p) >= kUpdRB * (kPcSamples + 2) * sizeof(double), "epilogue buffer");
    const RolloutArgs A = rollout_view<MODEL, BATCH, VARIED>(Ak);
    const int H = A.H;
    const int lane = threadIdx.x;
    stage_window<BATCH>(A, Wk, sh, kPcSamples);
    if (threadIdx.x < kMaxObst) obst_stage_form<FORM>(A, obst_lds, obst_mov, (int)threadIdx.x);
    // two-instruction clamps (clampd_fast, mppi_device_util.h): the host has checked sigma and the bounds, this wave the warm start;
    // a NaN anywhere takes every block through the compare-and-select instantiation.  (The staging is not an operand of the
    // `&&`: with A.fast_clamp off it would be skipped, and the kernel would read a warm start nobody put into LDS.)
    const bool nan_nominal = __builtin_amdgcn_ballot_w64(pc_stage_nominal<MODEL>(A, sh, kPcSamples)) != 0ull;
    const bool fast_clamp = A.fast_clamp && !nan_nominal;
    const int k = blockIdx.x * kPcSamples + lane;
    const bool live = k < A.K;
    const int kk = live ? k : A.K - 1;
    const uint32_t kg = (uint32_t)(A.k_offset + kk);
    double cost = 0.0;
    cost += pc_initial_cost<MODEL, MODE>(A);
    const int nblocks = (H + kTU - 1) / kTU;
    const int nstates = FB ? H - 2 : H;   // states that reach the path cost (dd:199 / fb:409)
    int prune_on = 1;
    PcState<MODEL> S;
    pc_initial_state<MODEL>(A, S);
    // (pc_produce_batched's flags of every block here: the wide-turn form, and a grid's gathers left for after the distance phase)
    constexpr unsigned WG = (WIDE ? kWideTurn : 0u) | (GRID ? kGridTaps : 0u);
    GridAcc grid_acc{};
    if constexpr (GRID) grid_acc = GridAcc{grid_row(A), 0.0, nstates, nullptr};
    __syncthreads();   // (one wave: the staged window and warm start are visible to all its lanes)
    // Wave priorities: two (or more) of these waves share a SIMD and run the same code in step; left alone they contend for
    // the same pipe at the same time.  Level (-rank - b) mod 4 -- the workgroup's dispatch rank on its CU, rotating with the
    // time block -- lets one run ahead for a block, then the other: C4 203.3 -> 191.1 us on one box (gpurun_out/r3by; the
    // other rotations tried there: (rank - b) 192.2, (rank - b / 2) 191.8, (rank + b) 194.0, two levels instead of four 195,
    // a constant level per wave: no gain, levels by phase (noise + dynamics high / distance low): +7 us).  CCV_MPPI_PRIO=0: off.
    const int prio_rank = A.prio_rotate ? (int)blockIdx.x / A.cu_count : 0;
    for (int b = 0; b < nblocks; ++b) {
        if (A.prio_rotate) pc_set_priority((-prio_rank - b) & 3);
        // ---------------- states and controls of steps 8b .. 8b+7
        bool done = false;
        GridTap tap[kTU];
        const int nctl = min(kTU, H - 1 - b * kTU);   // steps of this block that carry controls
        if (nctl == kTU) {
            if (fast_clamp)
                done = pc_produce_batched<MODEL, MODE, SoloShared<MODEL>, kFastClamp | WG>(A, sh, S, cost, b, lane, k, kk, live, kg, kNoNormalsAhead, kTU, &grid_acc, &tap);
            else if constexpr (!FB)   // (a second instantiation, so that a NaN in the warm start gives the multi-wave kernels'
                                      //  bits; full body has no registers for it -- its NaN case takes pc_produce below, whose
                                      //  sin / cos differ from the block path's in the last place)
                done = pc_produce_batched<MODEL, MODE, SoloShared<MODEL>, WG>(A, sh, S, cost, b, lane, k, kk, live, kg, kNoNormalsAhead, kTU, &grid_acc, &tap);
        } else if (nctl >= kPartialMin) {   // the horizon's last block, partly filled (C4: 7 of its 8 steps)
            if (fast_clamp)
                done = pc_produce_batched<MODEL, MODE, SoloShared<MODEL>, kPartialBlock | kFastClamp | WG>(A, sh, S, cost, b, lane, k, kk, live, kg, kNoNormalsAhead, nctl, &grid_acc, &tap);
            else if constexpr (!FB)
                done = pc_produce_batched<MODEL, MODE, SoloShared<MODEL>, kPartialBlock | WG>(A, sh, S, cost, b, lane, k, kk, live, kg, kNoNormalsAhead, nctl, &grid_acc, &tap);
        }
        if (!done) pc_produce<MODEL, MODE, false, GRID>(A, sh, S, cost, b, lane, k, kk, live, kg, &grid_acc);
        // ---------------- their distance to the window
        const int nv = min(kTU, nstates - b * kTU);
        pc_consume_states<MODEL, SoloShared<MODEL>, consume_discs(FORM)>(nv, A, sh, cost, b, lane, &prune_on, obst_lds, obst_mov);
        if constexpr (GRID) {
            if (done) grid_sum(grid_acc, tap, b * kTU);
        }
    }
    if constexpr (GRID) {
        if (grid_acc.row) cost = fma(grid_acc.row->w, grid_total(grid_acc), cost);   // the last term (section 10h)
    }
    if (A.prio_rotate) __builtin_amdgcn_s_setprio(0);
    // ---------------- weights and this wave's share of the update (dd:216-237)
    using Rows = UpdRowsT<kTU * udim_of(MODEL), 1>;
    const int R = (H - 1) * udim_of(MODEL);
    UpdT<MODE> upd[kUpdCH];
    const Rows rows{R, 0};
    const int mcount = A.fuse_update ? rows.count() : 0;
    if (mcount > 0) pc_update_fetch(A, upd, rows, 0, mcount, kk);   // (in flight during the exp below)
    const double total = cost;
    const double wgt = pc_weight<SHIFT>(A, total, live);
    if (live) {
        A.cost[k] = total;
        A.w[k] = wgt;
    }
    if (A.fuse_update) {
        pc_reduce_rows<kUpdRB, MODEL>(A, sh, &sh.p[0][0][0][0], upd, rows, mcount, wgt, lane, kk, fast_clamp);
        pc_block_stats(A, R, wgt, total, live, lane);
    }
}

}  // namespace ccv

// The producer half of the cooperative rollout kernels' building blocks: a lane's rollout state (PcState), the staging of the
// warm start, controls from normals, the state / normal stores, and a time block's sampling + dynamics + control costs, step
// by step (pc_produce) or as a batch (pc_produce_batched).
#pragma once
#include "fast_trig.h"
#include "mppi_cost_terms.h"
#include "mppi_device_util.h"
#include "mppi_kernels.h"
#include "noise_spec.h"

namespace ccv {

// element d of a 5-entry kernel-argument array for a compile-time d
template <int D>
__device__ __forceinline__ double arg5(const double (&v)[5]) { return v[D]; }

// lane state handed from the producer of block b to the producer of block b+1 (through LDS)
template <int MODEL>
struct PcState {
    double x, y, yaw;
    double roll, pitch;                                 // full body only
    double p_v, p_rv, p_sdir, p_cdir, p_c2, p_c3, p_ac;  // full body: step t-1 quantities for the ZMP term (fb:468-486)
    double sn, cs;                                      // diff drive: sin / cos of yaw, advanced by rotation (pc_produce_batched)
};
// the state before step 0: the pose the kernel holds, nothing behind it.  (Fills a reference: returned by value, the kernels that
// declare S ahead of the branch that fills it -- k_rollout_pc, k_rollout_r4 -- compiled to other instructions.)
template <int MODEL>
__device__ __forceinline__ void pc_initial_state(const RolloutArgs& A, PcState<MODEL>& S) {
    S.x = A.x0[0];
    S.y = A.x0[1];
    S.yaw = A.x0[2];
    S.roll = A.x0[3];
    S.pitch = A.x0[4];
    S.p_v = S.p_rv = S.p_sdir = S.p_c2 = S.p_c3 = S.p_ac = 0.0;
    S.p_cdir = 1.0;
    fast_sincos(A.x0[2], S.sn, S.cs);
}
// the cost every sample starts with: the full body's heading term of the first state, fb:408 -- identical for every sample
// (SURVEY.md Q15); nothing for the other models and where no cost is formed
template <int MODEL, int MODE>
__device__ __forceinline__ double pc_initial_cost(const RolloutArgs& A) {
    if constexpr (MODEL == CCV_MPPI_FULL_BODY && MODE != MODE_ROLLOUT) return A.w_yaw * (A.x0[2] - A.yaw_ref0) * (A.x0[2] - A.yaw_ref0);
    else return 0.0;
}

// The warm start u* is staged in LDS once per workgroup.  Read straight from memory inside the time loop (scalar or
// vector loads) every block of 8 steps exposes one cache-miss latency -- ~1500 cycles, measured -- on the producer chain.
// Returns whether one of the values this thread staged is NaN (see clampd_fast).
template <int MODEL, class SH>
__device__ __forceinline__ bool pc_stage_nominal(const RolloutArgs& A, SH& sh, const int nthreads,
                                                 const int tid = threadIdx.x) {   // (tid: 0 .. nthreads-1)
    const int R = (A.H - 1) * udim_of(MODEL);
    bool bad = false;
    if (A.pending_vec) {
        // K sharded over devices: the all-reduced [sum w, sum w*u] has not been divided yet -- do it here (the division
        // k_apply_partials would do, bit for bit) instead of spending a kernel launch on 100 quotients
        const double S = A.pending_vec[0];
        for (int j = tid; j < R + kTU * udim_of(MODEL); j += nthreads) {
            const double v = j < R ? A.pending_vec[1 + j] / S : 0.0;
            sh.nom[j] = v;
            bad |= v != v;
            if (blockIdx.x == 0 && j < R) {
                A.nominal_w[j] = v;
                A.nominal_used[j] = v;
            }
        }
        if (blockIdx.x == 0 && tid == 0) A.stats_w[0] = S;
        return bad;
    }
    for (int j = tid; j < R + kTU * udim_of(MODEL); j += nthreads) {
        const double v = j < R ? A.nominal[j] : 0.0;
        sh.nom[j] = v;
        bad |= v != v;
        if (blockIdx.x == 0 && j < R) A.nominal_used[j] = v;   // (the normals are stored, not the controls: kept with them)
    }
    return bad;
}

// The control of row n = t * u_dim + d from its normal: the samplers' arithmetic (double(z) * sigma + mean, clamp, steer_off),
// so the same bits as the value the rollout used.  D = n % u_dim is a template argument: the clamp bounds then are scalar
// kernel arguments (a run-time dimension would cost an integer division and two LDS reads with their waits per value).
template <int MODEL, int D, bool FASTCLAMP = false>
__device__ __forceinline__ double pc_control_from_normal_at(const RolloutArgs& A, const float z, const double nominal) {
    double v = (double)z * A.sigma + nominal;
    v = clampd_as<FASTCLAMP>(v, arg5<D>(A.umin), arg5<D>(A.umax));
    if constexpr (MODEL == CCV_MPPI_FULL_BODY && D == 2) {
        if (A.steer_off) v = 0.0;   // fb:517
    }
    return v;
}
template <int MODEL, int D, bool FASTCLAMP = false, class SH>
__device__ __forceinline__ double pc_control_from_normal(const RolloutArgs& A, const SH& sh, const float z, const int n) {
    return pc_control_from_normal_at<MODEL, D, FASTCLAMP>(A, z, sh.nom[n]);
}

// The candidate states x, y are written once and not read again by this kernel: streaming (non-temporal) stores keep
// them from displacing the controls, which the epilogue re-reads, from L2 and from piling up as dirty lines that the
// end-of-kernel write-back has to drain.
#define CCV_STATE_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))

// Stores with a scalar base: address = (uniform 64-bit row pointer) + (32-bit lane offset).  The compiler hoists the
// zero-extension of the lane offset out of the loop and then adds 64-bit vector addresses (one v_lshl_add_u64 per store,
// 198 per workgroup at C2); written out, a store issues no vector instruction for its address.  The compiler does not count
// these among the outstanding vector-memory operations: its own s_waitcnt vmcnt(n) then waits for more than it needs to, never
// for less (the counter covers them and operations complete in order), and the four-wave kernel's store wave counts its own.
// The row pitch in bytes stays below 4 GB by construction (32-bit lane offsets).  Used by the four-wave kernel's store wave
// (C2 -0.3 us, C3 -1.2 us); in the one-wave kernels the row pointers cost scalar registers they do not have (full body:
// 97 spilled SGPRs, 229.7 -> 232.0 us), so those keep the compiler's addressing.
__device__ __forceinline__ void pc_store_f32(char* const row, const uint32_t lane_off, const float v) {
    asm volatile("global_store_dword %0, %1, %2" ::"v"(lane_off), "v"(v), "s"(row) : "memory");
}
__device__ __forceinline__ void pc_store_f64_stream(char* const row, const uint32_t lane_off, const double v) {   // (non-temporal)
    asm volatile("global_store_dwordx2 %0, %1, %2 nt" ::"v"(lane_off), "v"(v), "s"(row) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------
// producer: steps t0 .. t0+7 of one sample (sampling + predict_NextState + control costs).  FULL: every step of the
// block carries controls (t0 + 8 <= H - 1), so the body is branch-free.
// ---------------------------------------------------------------------------------------------------------------
// GRID (the one-wave kernel's grid forms): every state of the block is looked up in the instance's occupancy grid as it is
// stored (grid_tap, mppi_cost_terms.h) and summed into *ga at once -- this is the rare path
template <int MODEL, int MODE, bool FULL, bool GRID = false, class SH>
__device__ __forceinline__ void pc_produce(const RolloutArgs& A, SH& sh, PcState<MODEL>& S, double& cost,
                                           const int b, const int lane, const int k, const int kk, const bool live,
                                           const uint32_t kg, GridAcc* ga = nullptr) {
    constexpr int UD = udim_of(MODEL);
    constexpr bool FB = MODEL == CCV_MPPI_FULL_BODY;
    constexpr bool COST = MODE != MODE_ROLLOUT;
    const int H = A.H;
    const int t0 = b * kTU;
    const size_t pitch = (size_t)A.pitch;
    const double dt = A.dt;
    float zq[4] = {0.f, 0.f, 0.f, 0.f};
    double4 nom = make_double4(0.0, 0.0, 0.0, 0.0);
    static_for<kTU>([&](auto TT) {
        constexpr int tt = decltype(TT)::value;
        const int t = t0 + tt;
        if constexpr (SH::kStage) {   // absolute: the store wave writes them out, the distance wave subtracts the pose
            sh.p[b & (SH::kPBuf - 1)][tt][0][lane] = S.x;
            sh.p[b & (SH::kPBuf - 1)][tt][1][lane] = S.y;
        } else {
            sh.p[b & (SH::kPBuf - 1)][tt][0][lane] = S.x - A.x0[0];
            sh.p[b & (SH::kPBuf - 1)][tt][1][lane] = S.y - A.x0[1];
        }
        if constexpr (GRID) {
            const double gx[1] = {S.x}, gy[1] = {S.y};
            GridTap tap[1];
            grid_issue(*ga, gx, gy, tap);
            grid_sum(*ga, tap, t);
        }
        if (FULL || t < H) {
            if constexpr (MODE != MODE_COST && !SH::kStage) {
                if (A.store_xy && live) {
                    CCV_STATE_STORE(&A.xs[(size_t)t * pitch + k], S.x);
                    CCV_STATE_STORE(&A.ys[(size_t)t * pitch + k], S.y);
                }
            }
            if (FULL || t < H - 1) {
                double u[UD];
                static_for<UD>([&](auto D) {
                    constexpr int d = decltype(D)::value;
                    constexpr int nloc = tt * UD + d;
                    const int n = t0 * UD + nloc;   // row = step*UD + dim
                    if constexpr (MODE == MODE_FUSED) {
                        if constexpr ((nloc & 3) == 0) {
                            // warm start u*[n .. n+3]: wave-uniform load, in flight while the Philox rounds run
                            nom = *reinterpret_cast<const double4*>(&sh.nom[n]);
                            const Philox4 r = philox4x32_10(kg, (uint32_t)(n >> 2), A.iter_lo, A.iter_hi, A.seed_lo, A.seed_hi);
                            box_muller_f32(r.x, r.y, zq[0], zq[1]);
                            box_muller_f32(r.z, r.w, zq[2], zq[3]);
                        }
                        constexpr int q = nloc & 3;
                        const double mean = q == 0 ? nom.x : q == 1 ? nom.y : q == 2 ? nom.z : nom.w;
                        // libstdc++ normal_distribution: ret * stddev + mean (dd:96-97), then clamp (dd:98-99)
                        double v = (double)zq[q] * A.sigma + mean;
                        v = clampd(v, arg5<d>(A.umin), arg5<d>(A.umax));
                        if constexpr (FB && d == 2) {
                            if (A.steer_off) v = 0.0;   // fb:517
                        }
                        u[d] = v;
                        if constexpr (SH::kStage) {
                            sh.zs[b & 1][nloc][lane] = zq[q];
                        } else {
                            if (live) A.z[(size_t)n * pitch + k] = zq[q];
                        }
                    } else {
                        u[d] = A.u[(size_t)n * pitch + kk];
                    }
                });
                // ---- cost terms that do not need the window ----
                if constexpr (COST) {
                    if constexpr (!FB) {
                        const double dv = u[0] - A.v_ref;
                        cost = fma(A.w_v * dv, dv, cost);   // dd:204-206 (the arithmetic of pc_produce_batched)
                    } else {
                        if (t < H - 2) {                                          // fb:409
                            cost += A.w_v * (u[0] - A.v_ref) * (u[0] - A.v_ref);  // fb:413
                            if (u[0] < 0.0) cost += A.w_back * u[0] * u[0];       // fb:420
                        }
                        if (t >= 1) {   // finish index t-1 <= H-3: ZMP (fb:468-485, 597-603) and roll-rate terms
                            const double mgz = A.fb_mass * A.fb_gz;                               // (mass*gravity_).z
                            const double drive_accel = div_uniform(u[0] - S.p_v, dt, A.inv_dt);   // fb:469
                            const double ay = drive_accel * S.p_sdir + S.p_ac * S.p_cdir;         // fb:473
                            const double hgdot_x = div_uniform(A.fb_Ixx * u[3] - A.fb_Ixx * S.p_rv, dt, A.inv_dt);   // fb:479-481
                            const double mo_x = (S.p_c2 * mgz + S.p_c3 * (A.fb_mass * ay)) - hgdot_x;  // fb:600
                            const double zmp_y = mo_x / mgz;                                      // fb:601 (accel.z == 0)
                            cost += A.w_zmp * zmp_y * zmp_y;                                      // fb:416
                            cost += A.w_rollv * (u[3] - S.p_rv) * (u[3] - S.p_rv);                // fb:418
                        }
                    }
                }
                // ---- dynamics: explicit Euler (dd:104-109, sd:120-125, fb:445-452) ----
                double hd = S.yaw;
                if constexpr (MODEL != CCV_MPPI_DIFF_DRIVE) hd = S.yaw + u[2];
                double sn, cs;
                fast_sincos(hd, sn, cs);
                if constexpr (FB && COST) {
                    double sd_, cd_, sr_, cr_, sp_, cp_;
                    fast_sincos(u[2], sd_, cd_);
                    fast_sincos(S.roll, sr_, cr_);
                    fast_sincos(S.pitch, sp_, cp_);
                    S.p_sdir = sd_;
                    S.p_cdir = cd_;
                    S.p_c2 = -A.fb_L * sr_;                    // CoM.y (fb:482)
                    S.p_c3 = A.fb_L * cp_ * cr_;               // CoM.z
                    S.p_ac = u[0] * u[1];                      // fb:471
                    S.p_v = u[0];
                    S.p_rv = u[3];
                }
                if constexpr (FB) {
                    S.x = S.x + u[0] * cs * dt;
                    S.y = S.y + u[0] * sn * dt;
                } else {   // (the arithmetic of pc_produce_batched)
                    const double step = u[0] * dt;
                    S.x = fma(step, cs, S.x);
                    S.y = fma(step, sn, S.y);
                }
                S.yaw = S.yaw + u[1] * dt;
                if constexpr (FB) {
                    S.roll = S.roll + u[3] * dt;
                    S.pitch = S.pitch + u[4] * dt;
                }
            } else {
                if constexpr (!FB && COST) {
                    // t == H-1: the reference reads control index H-1, one past the end (dd:199,204): defined as 0.0 (Q1)
                    const double dv = 0.0 - A.v_ref;
                    cost = fma(A.w_v * dv, dv, cost);
                }
            }
        }
    });
}

// The 4*CN normals of Philox calls C0 .. C0+CN-1 of time block b (call c holds normals 4c .. 4c+3 of the block): CN Philox
// blocks with their rounds interleaved, then the 2*CN Box-Muller pairs stage by stage.
template <int MODEL, int C0, int CN>
__device__ __forceinline__ void pc_block_normals(const RolloutArgs& A, const int b, const uint32_t kg, float (&z)[4 * CN]) {
    constexpr int UD = udim_of(MODEL);
    uint32_t c0[CN], c1[CN], c2[CN], c3[CN];
#pragma unroll
    for (int i = 0; i < CN; ++i) {
        c0[i] = kg;
        c1[i] = (uint32_t)((b * kTU * UD) >> 2) + (uint32_t)(C0 + i);
        c2[i] = A.iter_lo;
        c3[i] = A.iter_hi;
    }
    philox4x32_10_n<CN>(c0, c1, c2, c3, A.seed_lo, A.seed_hi);
    uint32_t ba[2 * CN], bb[2 * CN];
    float z0[2 * CN], z1[2 * CN];
#pragma unroll
    for (int i = 0; i < CN; ++i) {
        ba[2 * i] = c0[i];
        bb[2 * i] = c1[i];
        ba[2 * i + 1] = c2[i];
        bb[2 * i + 1] = c3[i];
    }
    box_muller_f32_n<2 * CN>(ba, bb, z0, z1);
#pragma unroll
    for (int i = 0; i < 2 * CN; ++i) {
        z[2 * i] = z0[i];
        z[2 * i + 1] = z1[i];
    }
}

// Full body, two-wave kernel: the producer (10 Philox calls, 20 Box-Muller pairs, 32 sin/cos per block) takes 1.5x as
// long as the distance phase of its partner, which then idles.  The partner therefore makes the first kPcAheadCalls
// Philox calls' normals of the block IT will produce next and parks them in LDS (its own slot: no synchronisation).
constexpr int kPcAheadCalls = 4;
template <int MODEL>
__device__ __forceinline__ void pc_noise_ahead(const RolloutArgs& A, float (*slot)[kPcSamples], const int b, const int lane,
                                               const uint32_t kg) {
    float z[4 * kPcAheadCalls];
    pc_block_normals<MODEL, 0, kPcAheadCalls>(A, b, kg, z);
#pragma unroll
    for (int i = 0; i < 4 * kPcAheadCalls; ++i) slot[i][lane] = z[i];
}

// The Philox calls of a time block in the groups they are made in (rounds interleaved within a group, then the group's
// Box-Muller pairs stage by stage): 4 | 3+3 | 4+3+3 by u_dim, the full body's first group being the one its partner wave may
// have made ahead.  f(C0, CN) once per group, C0 the group's first call and CN its calls, as integral constants.  A normal does
// not depend on the grouping.
template <int MODEL, class F>
__device__ __forceinline__ void pc_for_call_groups(F&& f) {
    constexpr int NCALL = kTU * udim_of(MODEL) / 4;
    using std::integral_constant;
    if constexpr (NCALL == 4) {
        f(integral_constant<int, 0>{}, integral_constant<int, 4>{});
    } else if constexpr (NCALL == 6) {
        f(integral_constant<int, 0>{}, integral_constant<int, 3>{});
        f(integral_constant<int, 3>{}, integral_constant<int, 3>{});
    } else {
        static_assert(NCALL == 10 && kPcAheadCalls == 4, "full body: 4 + 3 + 3 Philox calls");
        f(integral_constant<int, 0>{}, integral_constant<int, 4>{});
        f(integral_constant<int, 4>{}, integral_constant<int, 3>{});
        f(integral_constant<int, 7>{}, integral_constant<int, 3>{});
    }
}

// ---------------------------------------------------------------------------------------------------------------
// producer, fast path for a block whose 8 steps all carry controls: the same arithmetic as pc_produce, arranged in
// batches so that the independent chains of the 8 steps (Philox rounds, Box-Muller, sin/cos) sit in ONE basic block and
// interleave -- a lone wave then issues back to back instead of waiting out each chain's latency.
// ---------------------------------------------------------------------------------------------------------------
// FORM is a set of ProduceForm flags:
// kNormalsInLds (four-wave kernel): the block's normals are already in sh.zs, made by the noise wave.
// kFastClamp: the two-instruction clamp (clampd_fast, mppi_device_util.h: when it is allowed).
// kWideTurn (diff drive): sin / cos of every heading evaluated in full (fast_sincos_n, as steering does) instead of advanced by
// the step's turn -- for loop periods beyond |w|max dt = pi/4, where the short polynomials of the rotation form are not
// valid (the node measures dt, dd:346-348: one slow tick must not cost a different, twice as slow kernel).
// kPartialBlock: the horizon's last block when fewer than 8 of its steps carry controls (nctl = H - 1 - 8 b of them, 1 .. 7; the
// block's states are t0 .. t0 + nctl, the last one t = H - 1).  The whole batch is computed as for a full block -- the normals
// past row (H-1) u_dim are drawn and dropped, the warm start reads as 0 there -- and only what leaves the block is masked:
// stores, cost terms (dd / sd: the Q1 phantom term at t = H - 1), the step-range conditions of the full-body terms.  The
// reference defaults run H = 15: six of fourteen control steps used to go through the step-by-step path (pc_produce), whose
// chains (Philox -> Box-Muller -> sin/cos -> position, one step after the other) a lone wave waits out one by one.
// (worth it from kPartialMin steps on: a block of one or two steps is quicker step by step than as a batch of eight -- C2's
//  H - 1 = 49 leaves one step, and batching it cost the four-wave kernel 1.6 us)
// NCTL > 0 (with kPartialBlock): the number of control steps is known at compile time -- every mask folds, and what the masked steps
// would have computed falls away as dead code (the reference's default horizon H = 15 leaves a last block of six: a quarter of
// the batch).  The steps that remain are computed as before, bit for bit.
// kGridSum / kGridTaps (the one-wave kernel's grid forms; neither: no grid): the block's eight states are looked up in the
// instance's occupancy grid where they are stored, all gathers issued together; kGridSum: summed into *ga here; kGridTaps: left
// in *tap for the caller to sum after the distance phase (grid_sum), so that the gathers' latency passes under it
enum ProduceForm : unsigned { kNormalsInLds = 1u, kFastClamp = 2u, kWideTurn = 4u, kPartialBlock = 8u, kGridSum = 16u, kGridTaps = 32u };
// the "none" of the run-time argument `ahead`, by name: every Philox call of the block is made (or, kNormalsInLds, found) here
constexpr std::nullptr_t kNoNormalsAhead = nullptr;
template <int MODEL, int MODE, class SH, unsigned FORM = 0u, int NCTL = 0>
__device__ __forceinline__ bool pc_produce_batched(const RolloutArgs& A, SH& sh, PcState<MODEL>& S, double& cost,
                                                   const int b, const int lane, const int k, const int kk, const bool live,
                                                   const uint32_t kg,
                                                   const float (*ahead)[kPcSamples] = kNoNormalsAhead,   // pc_noise_ahead's slot
                                                   const int nctl_in = kTU,   // kPartialBlock without NCTL: the block's control steps
                                                   GridAcc* ga = nullptr, GridTap (*tap)[kTU] = nullptr) {   // kGridSum / kGridTaps
    constexpr bool ZLDS = (FORM & kNormalsInLds) != 0, FASTCLAMP = (FORM & kFastClamp) != 0, WIDE = (FORM & kWideTurn) != 0,
                   PARTIAL = (FORM & kPartialBlock) != 0;
    constexpr int GRID = (FORM & kGridSum) ? 1 : ((FORM & kGridTaps) ? 2 : 0);
    static_assert(NCTL == 0 || (PARTIAL && NCTL < kTU), "a compile-time step count is a partial block's");
    const int nctl = NCTL > 0 ? NCTL : (PARTIAL ? nctl_in : kTU);   // steps of this block that carry controls (wave-uniform)
    constexpr int UD = udim_of(MODEL);
    constexpr bool FB = MODEL == CCV_MPPI_FULL_BODY;
    constexpr bool COST = MODE != MODE_ROLLOUT;
    constexpr int NCALL = kTU * UD / 4;
    const int H = A.H;
    const int t0 = b * kTU;
    const size_t pitch = (size_t)A.pitch;
    const double dt = A.dt;
    // ---- 1. controls of the 8 steps
    double u[kTU][UD];
    if constexpr (MODE == MODE_FUSED) {
        // Philox calls in groups (rounds interleaved within a group, then the group's Box-Muller pairs stage by stage):
        // 4 | 3+3 | 5+5, or for full body 4 (possibly made ahead by the partner wave) + 3 + 3 (pc_for_call_groups)
        pc_for_call_groups<MODEL>([&](auto C0_, auto CN_) {
            constexpr int C0 = decltype(C0_)::value, CN = decltype(CN_)::value;
            const bool from_lds = NCALL == 10 && C0 == 0 && ahead != nullptr;   // (the full body's first group)
            float z[4 * CN];
            double nomv[4 * CN];   // warm start u* of this group from LDS (broadcast reads), in flight under the Philox rounds
#pragma unroll
            for (int i = 0; i < 4 * CN; ++i) nomv[i] = sh.nom[t0 * UD + 4 * C0 + i];
            CCV_KEEP_ORDER();
            if constexpr (ZLDS) {
#pragma unroll
                for (int i = 0; i < 4 * CN; ++i) z[i] = sh.zs[b & 1][4 * C0 + i][lane];
            } else if (from_lds) {
#pragma unroll
                for (int i = 0; i < 4 * CN; ++i) z[i] = ahead[4 * C0 + i][lane];
            } else {
                pc_block_normals<MODEL, C0, CN>(A, b, kg, z);
            }
            static_for<4 * CN>([&](auto II) {
                constexpr int i = decltype(II)::value;
                constexpr int nloc = 4 * C0 + i;
                constexpr int tt = nloc / UD, d = nloc % UD;
                // libstdc++ normal_distribution: ret * stddev + mean (dd:96-97), then clamp (dd:98-99)
                double v = (double)z[i] * A.sigma + nomv[i];
                v = clampd_as<FASTCLAMP>(v, arg5<d>(A.umin), arg5<d>(A.umax));
                if constexpr (FB && d == 2) {
                    if (A.steer_off) v = 0.0;   // fb:517
                }
                u[tt][d] = v;
                if constexpr (SH::kStage) {
                    if constexpr (!ZLDS) sh.zs[b & 1][nloc][lane] = z[i];   // (ZLDS: the noise wave has put it there)
                } else {
                    // no `live` predicate: rows are padded to a multiple of 64 samples (pitch), lanes past K write their
                    // padding slot -- a branch per store would cut this block into pieces the scheduler cannot interleave
                    if (!PARTIAL || tt < nctl) A.z[(size_t)(t0 * UD + nloc) * pitch + k] = z[i];
                }
            });
        });
    } else {
#pragma unroll
        for (int tt = 0; tt < kTU; ++tt)
#pragma unroll
            for (int d = 0; d < UD; ++d) u[tt][d] = (!PARTIAL || tt < nctl) ? A.u[(size_t)((t0 + tt) * UD + d) * pitch + kk] : 0.0;
    }
    // ---- 2. heading (roll, pitch) recurrences: yaw[t+1] = yaw[t] + w[t]*dt (dd:108, fb:449-451)
    double yawv[kTU + 1], rollv[FB ? kTU + 1 : 1], pitchv[FB ? kTU + 1 : 1];
    yawv[0] = S.yaw;
    if constexpr (FB) {
        rollv[0] = S.roll;
        pitchv[0] = S.pitch;
    }
#pragma unroll
    for (int tt = 0; tt < kTU; ++tt) {
        yawv[tt + 1] = yawv[tt] + u[tt][1] * dt;
        if constexpr (FB) {
            rollv[tt + 1] = rollv[tt] + u[tt][3] * dt;
            pitchv[tt + 1] = pitchv[tt] + u[tt][4] * dt;
        }
    }
    // (the host only selects this kernel when every reachable angle is inside the branch-free sin/cos range:
    //  ccv_mppi_capi.hip fast_trig_safe())
    double hd[kTU];
#pragma unroll
    for (int tt = 0; tt < kTU; ++tt) {
        hd[tt] = yawv[tt];
        if constexpr (MODEL != CCV_MPPI_DIFF_DRIVE) hd[tt] = yawv[tt] + u[tt][2];
    }
    // ---- 3. sin/cos of the 8 headings
    double sn[kTU], cs[kTU];
    double fb_sd[FB ? kTU : 1], fb_cd[FB ? kTU : 1], fb_sr[FB ? kTU : 1], fb_cr[FB ? kTU : 1], fb_cp[FB ? kTU : 1];   // full body: direction, roll, pitch
    if constexpr (MODEL == CCV_MPPI_DIFF_DRIVE && !WIDE) {
        // diff drive: the heading only ever changes by the step's turn w*dt, so its (sin, cos) are ADVANCED by that angle --
        // eight short independent polynomial pairs (no range reduction, no quadrant logic: the host admits this kernel
        // only for |w| dt <= pi/4) and a chain of eight 2x2 rotations, ~25 fp64 operations per step instead of ~40.
        // Rounding differs from sin(yaw) / cos(yaw) of the accumulated yaw by a few ulp per step.
        double turn[kTU], sd[kTU], cd[kTU];
#pragma unroll
        for (int tt = 0; tt < kTU; ++tt) turn[tt] = u[tt][1] * dt;
        kernel_sincos_n<kTU>(turn, sd, cd);
        double s_ = S.sn, c_ = S.cs;
#pragma unroll
        for (int tt = 0; tt < kTU; ++tt) {
            sn[tt] = s_;
            cs[tt] = c_;
            const double s2 = fma(s_, cd[tt], c_ * sd[tt]);
            const double c2 = fma(c_, cd[tt], -(s_ * sd[tt]));
            s_ = s2;
            c_ = c2;
        }
        if constexpr (NCTL == 0) {
            S.sn = s_;
            S.cs = c_;
        }
    } else if constexpr (FB) {
        // full body needs sin / cos of four angles per step: heading = yaw + direction, direction, roll, pitch.  Every one
        // of them either is small (|direction| <= pi/4: a clamped control) or changes by a small step (yaw, roll, pitch:
        // rate * dt; the host admits this kernel only for |rate| dt <= pi/4, fast_trig_safe()), so per block one full
        // evaluation of sin / cos(yaw), (roll), (pitch) at the block's first step is advanced by rotations, and the short
        // polynomials (no range reduction, no quadrant logic) do the rest: 32 batched short evaluations + 3 full ones per
        // block instead of 32 full ones.  sin / cos(yaw + direction) comes from the addition theorem.  Rounding differs
        // from the direct evaluation by a few ulp per step; the chains restart from the accumulated angles every block.
        double turn[kTU], st_[kTU], ct_[kTU], dir[kTU];
#pragma unroll
        for (int tt = 0; tt < kTU; ++tt) {
            turn[tt] = u[tt][1] * dt;
            dir[tt] = u[tt][2];
        }
        kernel_sincos_n<kTU>(turn, st_, ct_);
        kernel_sincos_n<kTU>(dir, fb_sd, fb_cd);
        double sy, cy;
        fast_sincos(yawv[0], sy, cy);
#pragma unroll
        for (int tt = 0; tt < kTU; ++tt) {
            sn[tt] = fma(sy, fb_cd[tt], cy * fb_sd[tt]);
            cs[tt] = fma(cy, fb_cd[tt], -(sy * fb_sd[tt]));
            const double s2 = fma(sy, ct_[tt], cy * st_[tt]);
            const double c2 = fma(cy, ct_[tt], -(sy * st_[tt]));
            sy = s2;
            cy = c2;
        }
        if constexpr (COST) {
            double rinc[kTU], pinc[kTU], sri[kTU], cri[kTU], spi[kTU], cpi[kTU];
#pragma unroll
            for (int tt = 0; tt < kTU; ++tt) {
                rinc[tt] = u[tt][3] * dt;
                pinc[tt] = u[tt][4] * dt;
            }
            kernel_sincos_n<kTU>(rinc, sri, cri);
            kernel_sincos_n<kTU>(pinc, spi, cpi);
            double sr, cr, sp, cp;
            fast_sincos(rollv[0], sr, cr);
            fast_sincos(pitchv[0], sp, cp);
#pragma unroll
            for (int tt = 0; tt < kTU; ++tt) {
                fb_sr[tt] = sr;
                fb_cr[tt] = cr;
                fb_cp[tt] = cp;
                const double s2 = fma(sr, cri[tt], cr * sri[tt]);
                const double c2 = fma(cr, cri[tt], -(sr * sri[tt]));
                sr = s2;
                cr = c2;
                const double s3 = fma(sp, cpi[tt], cp * spi[tt]);
                const double c3 = fma(cp, cpi[tt], -(sp * spi[tt]));
                sp = s3;
                cp = c3;
            }
        }
    } else {
        // independent chains, evaluated stage by stage in two groups of four
        constexpr int SG = 4;
#pragma unroll
        for (int g = 0; g < kTU / SG; ++g) {
            double xin[SG], so[SG], co[SG];
#pragma unroll
            for (int i = 0; i < SG; ++i) xin[i] = hd[g * SG + i];
            fast_sincos_n<SG>(xin, so, co);
#pragma unroll
            for (int i = 0; i < SG; ++i) {
                sn[g * SG + i] = so[i];
                cs[g * SG + i] = co[i];
            }
        }
    }
    // ---- 4. cost terms that do not need the window
    if constexpr (COST) {
        if constexpr (!FB) {
#pragma unroll
            for (int tt = 0; tt < kTU; ++tt) {
                // dd:204-206: v_weight (v - v_ref)^2, the last factor riding on the addition
                if constexpr (PARTIAL) {
                    // t == H-1: the reference reads control index H-1, one past the end (dd:199,204): defined as 0.0 (Q1)
                    const double dv = (tt < nctl ? u[tt][0] : 0.0) - A.v_ref;
                    cost = tt <= nctl ? fma(A.w_v * dv, dv, cost) : cost;
                } else {
                    const double dv = u[tt][0] - A.v_ref;
                    cost = fma(A.w_v * dv, dv, cost);
                }
            }
        } else {
            const double mgz = A.fb_mass * A.fb_gz;   // (mass*gravity_).z
#pragma unroll
            for (int tt = 0; tt < kTU; ++tt) {
                const int t = t0 + tt;
                // the two step-range conditions are wave-uniform: selects, not branches, keep the block in one piece
                {                                                                     // fb:409: t < H - 2
                    const double cv = A.w_v * (u[tt][0] - A.v_ref) * (u[tt][0] - A.v_ref);       // fb:413
                    const double cb = A.w_back * u[tt][0] * u[tt][0];                            // fb:420
                    const bool in = t < H - 2;
                    cost += in ? cv : 0.0;
                    cost += (in && u[tt][0] < 0.0) ? cb : 0.0;
                }
                {   // t >= 1: finish index t-1: ZMP (fb:468-485, 597-603) and roll-rate terms
                    const double drive_accel = div_uniform(u[tt][0] - S.p_v, dt, A.inv_dt);      // fb:469
                    const double ay = drive_accel * S.p_sdir + S.p_ac * S.p_cdir;                // fb:473
                    const double hgdot_x = div_uniform(A.fb_Ixx * u[tt][3] - A.fb_Ixx * S.p_rv, dt, A.inv_dt);   // fb:479-481
                    const double mo_x = (S.p_c2 * mgz + S.p_c3 * (A.fb_mass * ay)) - hgdot_x;    // fb:600
                    const double zmp_y = mo_x / mgz;                                             // fb:601
                    const double cz = A.w_zmp * zmp_y * zmp_y;                                   // fb:416
                    const double cr = A.w_rollv * (u[tt][3] - S.p_rv) * (u[tt][3] - S.p_rv);     // fb:418
                    const bool in = t >= 1 && (!PARTIAL || tt < nctl);   // (index t-1 <= H-3)
                    cost += in ? cz : 0.0;
                    cost += in ? cr : 0.0;
                }
                if (NCTL == 0 || tt < NCTL) {   // (a compile-time count: nothing reads the state past the last control step)
                    S.p_sdir = fb_sd[tt];
                    S.p_cdir = fb_cd[tt];
                    S.p_c2 = -A.fb_L * fb_sr[tt];                 // CoM.y (fb:482)
                    S.p_c3 = A.fb_L * fb_cp[tt] * fb_cr[tt];      // CoM.z
                    S.p_ac = u[tt][0] * u[tt][1];       // fb:471
                    S.p_v = u[tt][0];
                    S.p_rv = u[tt][3];
                }
            }
        }
    }
    // ---- 5. positions (dd:106-107), hand-off of (x,y) - pose to the consumer, x,y -> HBM
    double x = S.x, y = S.y;
    double xv[kTU], yv[kTU];
#pragma unroll
    for (int tt = 0; tt < kTU; ++tt) {
        xv[tt] = x;
        yv[tt] = y;
        if (NCTL == 0 || tt <= NCTL) {   // (a compile-time count: the states past t = H - 1 are nobody's)
            if constexpr (SH::kStage) {
                sh.p[b & (SH::kPBuf - 1)][tt][0][lane] = x;
                sh.p[b & (SH::kPBuf - 1)][tt][1][lane] = y;
            } else {
                sh.p[b & (SH::kPBuf - 1)][tt][0][lane] = x - A.x0[0];
                sh.p[b & (SH::kPBuf - 1)][tt][1][lane] = y - A.x0[1];
            }
        }
        if constexpr (FB) {
            // (the full-body kernels keep the reference's form: the one-wave kernel sits at 256 registers, and every
            //  rearrangement of this block tried so far -- fused products here or in the cost terms, weights switched instead
            //  of 64-bit selects -- either spills or costs it 4 - 14 us of C4's 206, profiles/README.md round 3)
            x = x + u[tt][0] * cs[tt] * dt;
            y = y + u[tt][0] * sn[tt] * dt;
        } else {
            const double step = u[tt][0] * dt;   // dd:106-107: x + v cos(yaw) dt -- one product shared, the other fused
            x = fma(step, cs[tt], x);
            y = fma(step, sn[tt], y);
        }
    }
    if constexpr (MODE != MODE_COST && !SH::kStage) {
        if (A.store_xy) {   // one wave-uniform branch for the 16 stores (padded rows: no `live` predicate, as above)
#pragma unroll
            for (int tt = 0; tt < kTU; ++tt) {
                if (!PARTIAL || tt <= nctl) {   // states t <= H-1
                    CCV_STATE_STORE(&A.xs[(size_t)(t0 + tt) * pitch + k], xv[tt]);
                    CCV_STATE_STORE(&A.ys[(size_t)(t0 + tt) * pitch + k], yv[tt]);
                }
            }
        }
    }
    if constexpr (GRID == 1) {
        GridTap here[kTU];
        grid_issue(*ga, xv, yv, here);
        grid_sum(*ga, here, t0);
    } else if constexpr (GRID == 2) {
        grid_issue(*ga, xv, yv, *tap);
    }
    if constexpr (NCTL > 0) return true;   // (the horizon's last block: the state is not carried any further)
    S.x = x;
    S.y = y;
    S.yaw = yawv[kTU];
    if constexpr (FB) {
        S.roll = rollv[kTU];
        S.pitch = pitchv[kTU];
    }
    return true;
}

}  // namespace ccv

// The fused-update epilogue of the cooperative rollout kernels: a sample's weight, the workgroup's share of sum w and sum w u
// per control row (pc_reduce_rows) and its cost statistics (pc_block_stats).
#pragma once
#include "mppi_device_util.h"
#include "mppi_kernels.h"
#include "mppi_produce.h"

namespace ccv {

// ---------------------------------------------------------------------------------------------------------------
// Fused first half of determine_OptimalSolution() (dd:228-237): this workgroup's share of sum_i w_i and
// sum_i w_i * u_i[t][d] for every control row, so that the K x (H-1) x u_dim controls are not streamed from HBM a second
// time by a separate kernel -- they are re-read here, by the CU that wrote them (L2 / Infinity Cache hits).
// Rows are dealt to the two waves; a wave reduces 15 rows at a time through LDS: every lane drops w*u for each row,
// then lane (r, q) adds 16 of the 64 entries of row r and two shuffles finish the row.  Fixed order => reproducible.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kUpdRB = 15;                  // rows per LDS batch: 15 * 66 doubles fit one wave's half of sh.p
constexpr int kUpdCH = 4 * kUpdRB;          // rows whose loads are in flight together (120 VGPRs)

// Control rows dealt to the waves of a workgroup in units of BR rows: wave w of NW owns units w, w+NW, ...
// m = 0 .. count()-1 enumerates a wave's rows.  k_rollout_pc: BR = rows of one time block, NW = 2, so that every wave
// re-reads exactly the rows it stored itself (program order makes them visible; no vector-memory wait at the barriers).
template <int BR_, int NW_>
struct UpdRowsT {
    static constexpr int BR = BR_, NW = NW_;
    int R, wv;
    __device__ __forceinline__ int count() const {
        int n = 0;
        for (int r0 = wv * BR; r0 < R; r0 += NW * BR) n += min(BR, R - r0);
        return n;
    }
    __device__ __forceinline__ int row(const int m) const { return ((m / BR) * NW + wv) * BR + m % BR; }
};

// The re-read of this workgroup's controls: the loads of a whole chunk of rows are issued back to back, so the chunk
// pays one memory latency, not one per batch.  Rows past the end are clamped (loaded, never used).
// T = float: the fused iteration stored the normals (A.z); T = double: the stage-wise calls hold the controls themselves (A.u)
template <int MODE>
using UpdT = std::conditional_t<MODE == MODE_FUSED, float, double>;
template <class T, class ROWS>
__device__ __forceinline__ void pc_update_fetch(const RolloutArgs& A, T (&v)[kUpdCH], const ROWS& rows, const int m0,
                                                const int mcount, const int kk) {
    const size_t pitch = (size_t)A.pitch;
#pragma unroll
    for (int i = 0; i < kUpdCH; ++i) {
        const size_t at = (size_t)rows.row(min(m0 + i, mcount - 1)) * pitch + kk;
        if constexpr (std::is_same<T, float>::value) v[i] = A.z[at];
        else v[i] = A.u[at];
    }
}

// sum_k w_k * u_k[row] over the 64 samples of the workgroup for this wave's rows -> A.partial[row][workgroup].
// RB rows at a time through the wave-private LDS buffer `buf` (RB * 65 doubles): every lane drops w*u for each row, then
// lane (r, q) adds 16 of the 64 entries of row r and two shuffles finish the row.  (The caller has fetched the first
// chunk into v.)
// LOOP (four-wave kernel): the batches of a chunk are a real loop whose body always works on v[0 .. RB-1]; after a batch the
// register array is shifted down by RB (48 moves).  Unrolled, the epilogue is 2-3 KB of straight-line code per wave that runs
// once, and the instruction cache is cold for every line of it: tools/stamps_r4.py found 1.6 us per batch of 12 rows, the time
// of ~20 line fetches, not of 150 instructions.  (The one- and two-wave kernels go round their unrolled chunk several times.)
template <int RB, int MODEL, bool LOOP = false, class SH, class T, class ROWS>
__device__ __forceinline__ void pc_reduce_rows(const RolloutArgs& A, const SH& sh, double* buf, T (&v)[kUpdCH], const ROWS& rows,
                                               const int mcount, const double wgt, const int lane, const int kk,
                                               const bool fast_clamp = false) {   // (wave-uniform: see clampd_fast)
    static_assert(RB <= 16 && kUpdCH % RB == 0, "batch size");
    // A row is 64 products with one slot of padding after the first 32 (sample k at column k + (k >> 5)) and one at the end:
    // lane (r, q) then reads its 16 entries of row r from banks that no other lane of its half-wave touches (with 65-double
    // rows the lanes q and q + 2 of a row met in the same bank: every ds_read_b64 of the sums took two passes)
    constexpr int STRIDE = kPcSamples + 2;
    const int rr = lane >> 2, q = lane & 3;
    const int col_w = lane + (lane >> 5), col_r = q * 16 + (q >> 1);
    // one batch: products of rows base .. base+RB-1 (held in v[V0 .. V0+RB-1]) -> LDS -> row sums -> partial
    auto batch = [&](auto V0_, const int base) {
        constexpr int V0 = decltype(V0_)::value;
        const int nrows = min(RB, mcount - base);
        // the warm start of the batch's rows first, all reads in flight together: read row by row between the LDS writes
        // below, every row waits out an LDS round trip (the compiler keeps LDS reads behind LDS writes: 12 x lgkmcnt(0) per
        // batch, ~1.6 us per batch with sixteen waves of a CU in their epilogues at once)
        double nomv[RB];
        if constexpr (std::is_same<T, float>::value) {
#pragma unroll
            for (int r = 0; r < RB; ++r) nomv[r] = sh.nom[rows.row(min(base + r, mcount - 1))];
        }
        auto products = [&](auto FAST_) {
            constexpr bool FAST = decltype(FAST_)::value;
            static_for<RB>([&](auto RR) {
                constexpr int r = decltype(RR)::value;
                if constexpr (std::is_same<T, float>::value) {
                    // the row's control dimension: rows are dealt in units of ROWS::BR (a multiple of u_dim), chunks of kUpdCH
                    // (= 60: a multiple of 2, 3 and 5) and batches of RB, so it only depends on the position inside the batch
                    constexpr int UD = udim_of(MODEL);
                    static_assert(ROWS::BR % UD == 0 && kUpdCH % UD == 0 && (!LOOP || RB % UD == 0), "row dealing vs control dimension");
                    constexpr int d = (V0 + r) % UD;
                    // (rows past the end: clamped above, never summed)
                    buf[r * STRIDE + col_w] = wgt * pc_control_from_normal_at<MODEL, d, FAST>(A, v[V0 + r], nomv[r]);
                } else {
                    buf[r * STRIDE + col_w] = wgt * v[V0 + r];
                }
            });
        };
        if (std::is_same<T, float>::value && fast_clamp) products(std::true_type{});
        else products(std::false_type{});
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS writes have landed (wave-private buffer)
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        if (rr < nrows) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc += buf[rr * STRIDE + col_r + i];
        }
        acc += dpp_move<kDppXor1>(acc);   // the four lanes of a row are one quad
        acc += dpp_move<kDppXor2>(acc);
        if (rr < nrows && q == 0) A.partial[(size_t)rows.row(base + rr) * A.nparts + blockIdx.x] = acc;
        __builtin_amdgcn_wave_barrier();
    };
    for (int chunk0 = 0; chunk0 < mcount; chunk0 += kUpdCH) {
        if (chunk0 != 0) pc_update_fetch(A, v, rows, chunk0, mcount, kk);
        if constexpr (LOOP) {
#pragma clang loop unroll(disable)
            for (int base = chunk0; base < min(mcount, chunk0 + kUpdCH); base += RB) {
                batch(std::integral_constant<int, 0>{}, base);
#pragma unroll
                for (int i = 0; i + RB < kUpdCH; ++i) v[i] = v[i + RB];
            }
        } else {
            static_for<kUpdCH / RB>([&](auto BB) {
                constexpr int bb = decltype(BB)::value;
                if (chunk0 + bb * RB < mcount) batch(std::integral_constant<int, bb * RB>{}, chunk0 + bb * RB);
            });
        }
    }
}

// sum of weights + cost statistics of the workgroup (one wave)
__device__ __forceinline__ void pc_block_stats(const RolloutArgs& A, const int R, const double wgt, const double total, const bool live,
                                               const int lane) {
    const double sw = wave_sum(wgt);
    const double mn = wave_min(live ? total : INFINITY);
    const double mx = wave_max(live ? total : -INFINITY);
    const double nz = wave_sum((live && wgt == 0.0) ? 1.0 : 0.0);
    if (lane == 0) {
        A.partial[(size_t)R * A.nparts + blockIdx.x] = sw;
        A.statpart[blockIdx.x * 3 + 0] = mn;
        A.statpart[blockIdx.x * 3 + 1] = mx;
        A.statpart[blockIdx.x * 3 + 2] = nz;
    }
}

// Shifted weights of a batch handle (ccv_mppi_batch_set_min_shift): relative to the minimum cost m_g of the workgroup's 64
// samples -- the value pc_block_stats posts as statpart[g][0], formed by the same reduction, so every wave that holds the
// workgroup's totals gets the same bits without a hand-off.  The best sample of the workgroup has weight exp(-0) = 1; the
// update rescales the workgroup's sums by exp(-(m_g - m) / lambda), m = the instance's minimum (k_finalize_batch_shift).
// A workgroup without a finite cost (m_g = +inf) keeps the unshifted form: its +inf costs weigh 0, a NaN cost stays NaN.
__device__ __forceinline__ double pc_shifted_weight(const RolloutArgs& A, const double total, const bool live) {
    const double mg = wave_min(live ? total : INFINITY);
    const double shift = mg < INFINITY ? mg : 0.0;
    return live ? exp(-(total - shift) / A.lambda) : 0.0;
}
// a sample's unnormalised weight: exp(-cost / lambda), dd:219 (no min-cost shift); SHIFT: the shifted form above
// (called by every wave of the workgroup: the same 64 totals, the same minimum); a lane past K weighs 0
template <bool SHIFT>
__device__ __forceinline__ double pc_weight(const RolloutArgs& A, const double total, const bool live) {
    if constexpr (SHIFT) return pc_shifted_weight(A, total, live);
    else return live ? exp(-total / A.lambda) : 0.0;
}

}  // namespace ccv

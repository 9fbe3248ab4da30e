// The consumer half of the cooperative rollout kernels' building blocks: the exact pruning of the window for a wave's block of
// states (pc_prune_window) and the distance loop with the path cost and the obstacle terms (pc_consume).
#pragma once
#include "mppi_cost_terms.h"
#include "mppi_device_util.h"
#include "mppi_handoff.h"
#include "mppi_kernels.h"

namespace ccv {

// states of a block whose distance the distance wave computes; the store wave would take the rest.  8: measured best
// (6 + 2 is 4 us slower at K = 65 536: with eight waves per CU storing, the store wave is busy most of a block time)
constexpr int kConsumeStates = 8;

// ---------------------------------------------------------------------------------------------------------------
// Exact pruning of the window for one wave and one block of states.  f_j(p) = a_j px + b_j py + c_j (= |p - r_j|^2 - |p|^2)
// is linear in p, so is the difference of two of them: window point j cannot be the nearest one for ANY position p of the
// wave if some other point r DOMINATES it over a set that contains them all,
//     min over the box B of (f_j - f_r)(p)  =  (c_j - c_r) + min((a_j - a_r) x) + min((b_j - b_r) y)  >  0,
// i.e. B lies strictly on r's side of the bisector of r_j and r.  B is the bounding box of the wave's NV x 64 positions;
// the candidates r are the window points nearest to B's four corners.  Lanes take the role of window points; the
// survivors are contiguous along a path, so the distance loop runs over their hull.  On the launch workload 31 % of the
// (state, point) pairs remain (tools/prune_study.py; all-pairs dominance over the same boxes: 30 %, the hull of the true
// nearest points: 24 %), against 56 % for the round-1 test (one bound M = min_j max_B f_j against min_B f_j, which takes
// the two extrema at different corners).
// Nothing here assumes a path-like window: any point excluded is excluded by a valid inequality, the rest costs time only.
// Rounding: the box and the choice of r are made in fp32 (any r is a valid dominator; the box is rounded outwards), the
// inequality itself in fp64 against T = 1e-9 * (sum of the magnitudes that enter it) -- the rounding errors of the test and
// of the loop's own f_j(p), f_r(p) are below 1e-15 of that sum.  Everything unordered (NaN / infinite positions or
// coefficients) fails the comparison and keeps the point; a lane whose own position is not finite ends at the 100 m
// gate value whatever the loop covers.
// ---------------------------------------------------------------------------------------------------------------
template <int NV, int NHALF, class SH>   // NHALF: window points per lane (2 when the window is longer than 64)
__device__ __forceinline__ void pc_prune_window(const RolloutArgs& A, const SH& sh, const double (&px)[NV], const double (&py)[NV],
                                                const int lane, int& jb, int& je) {
    // ---- bounding box of the NV x 64 positions
    float xlo = (float)px[0], ylo = (float)py[0];
    float xhi = xlo, yhi = ylo;
#pragma unroll
    for (int i = 1; i < NV; ++i) {
        const float fx = (float)px[i], fy = (float)py[i];
        xlo = fminf(xlo, fx);
        xhi = fmaxf(xhi, fx);
        ylo = fminf(ylo, fy);
        yhi = fmaxf(yhi, fy);
    }
    wave_min_max_min_max_f32(xlo, xhi, ylo, yhi);
    // outwards: |x - (float)x| <= 2^-24 |x|, or 2^-126 where fp32 goes subnormal / flushes
    const double bx0 = (double)xlo - (fabs((double)xlo) * 1.2e-7 + 1.0e-37), bx1 = (double)xhi + (fabs((double)xhi) * 1.2e-7 + 1.0e-37);
    const double by0 = (double)ylo - (fabs((double)ylo) * 1.2e-7 + 1.0e-37), by1 = (double)yhi + (fabs((double)yhi) * 1.2e-7 + 1.0e-37);
    const double X = fmax(fabs(bx0), fabs(bx1)), Y = fmax(fabs(by0), fabs(by1));
    // ---- this lane's window points: j = lane, and lane + 64 when the window is longer than 64
    double2 ab[NHALF];
    double c[NHALF], tj[NHALF];
    float v[4][NHALF];
    bool valid[NHALF];
#pragma unroll
    for (int hh = 0; hh < NHALF; ++hh) {
        const int j = lane + 64 * hh;
        valid[hh] = j < A.H;
        ab[hh] = valid[hh] ? sh.ab[j] : make_double2(0.0, 0.0);
        c[hh] = valid[hh] ? sh.c[j] : INFINITY;
        tj[hh] = 1.0e-9 * (fabs(c[hh]) + (fabs(ab[hh].x) * X + fabs(ab[hh].y) * Y));
        // f_j at the four corners, fp32: only to choose the dominators
        const float a32 = (float)ab[hh].x, b32 = (float)ab[hh].y, c32 = (float)c[hh];
        v[0][hh] = __builtin_fmaf(a32, xlo, __builtin_fmaf(b32, ylo, c32));
        v[1][hh] = __builtin_fmaf(a32, xlo, __builtin_fmaf(b32, yhi, c32));
        v[2][hh] = __builtin_fmaf(a32, xhi, __builtin_fmaf(b32, ylo, c32));
        v[3][hh] = __builtin_fmaf(a32, xhi, __builtin_fmaf(b32, yhi, c32));
    }
    float best[4], mine[4];
    unsigned long long upper[4];   // lanes whose better candidate is lane + 64
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        upper[k] = 0ull;
        mine[k] = v[k][0];
        if constexpr (NHALF == 2) {
            const bool up = v[k][1] < v[k][0];
            upper[k] = __ballot(up);
            mine[k] = up ? v[k][1] : v[k][0];
        }
        best[k] = mine[k];
    }
    wave_min4_f32(best[0], best[1], best[2], best[3]);
    int jr[4];
    bool ok[4];
    double2 abr[4];
    double cr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long at = __ballot(mine[k] == best[k]);   // (empty when every value is NaN)
        ok[k] = at != 0ull;
        const int r = ok[k] ? __builtin_ctzll(at) : 0;
        jr[k] = r + (int)((upper[k] >> r) & 1ull) * 64;
        // (every valid lane NaN and the padding's +inf the minimum: jr = H, the padding -- for H a multiple of 4 below 64 the entry
        //  after it, which stage_window does not write; such a window is beyond fp32's range, every d^2 ends at the gate: DESIGN 13)
        abr[k] = sh.ab[jr[k]];   // wave-uniform address: broadcast reads, all four in flight together
        cr[k] = sh.c[jr[k]];
    }
    // ---- dominance of this lane's points by each of the four
    unsigned long long keep[2] = {0ull, 0ull};
#pragma unroll
    for (int hh = 0; hh < NHALF; ++hh) {
        bool kp = valid[hh];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double da = ab[hh].x - abr[k].x, db = ab[hh].y - abr[k].y, dc = c[hh] - cr[k];
            const double L = dc + (fmin(da * bx0, da * bx1) + fmin(db * by0, db * by1));
            const double T = tj[hh] + 1.0e-9 * (fabs(cr[k]) + (fabs(abr[k].x) * X + fabs(abr[k].y) * Y));
            kp = kp && !(ok[k] && L > T);
        }
        keep[hh] = __ballot(kp);
    }
    if (keep[0] | keep[1]) {
        const int lo = keep[0] ? __builtin_ctzll(keep[0]) : 64 + __builtin_ctzll(keep[1]);
        const int hi = keep[1] ? 127 - __builtin_clzll(keep[1]) : 63 - __builtin_clzll(keep[0]);
        jb = lo & ~3;
        je = (hi | 3) + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// consumer: min over the H window points of (a_j px + b_j py + c_j) for the NV states of one block, then the path cost.
// Straight fp64 FMA/MIN; four window points per iteration so the LDS broadcast reads are covered and the compiler's
// canonicalising max in front of fmin() is paid once per four minima.
// ---------------------------------------------------------------------------------------------------------------
// FORM is a set of ConsumeForm flags:
// kLeanRegisters (four-wave kernel, 128 VGPRs): two window points per register set instead of four and the running minimum taken
// point pair by point pair -- 48 registers less; the same minima, hence the same bits.
// kDiscs (batch handles, on VARIED): after the block's path terms, the instance's disc-obstacle term of the same states from the
// coefficients staged in `ob` (obst_term, mppi_cost_terms.h); the window pruning does not touch that list.
// kMovingDiscs (on kDiscs): the discs move -- the coefficients staged in `obm`, state i of block b at step b * kTU + i of the
// horizon (obst_term_moving)
enum ConsumeForm : unsigned { kLeanRegisters = 1u, kDiscs = 2u, kMovingDiscs = 4u };
// the disc flags of a kernel of rung `form` (BatchForm, mppi_kernels.h)
__host__ __device__ constexpr unsigned consume_discs(const BatchForm form) {
    return form >= BatchForm::Moving ? (kDiscs | kMovingDiscs) : (form >= BatchForm::Obst ? kDiscs : 0u);
}
// the "none" of the run-time arguments `ob` / `obm`, by name (a kernel below the rung Obst that hands over a sequence number)
constexpr std::nullptr_t kNoDiscs = nullptr;
template <int NV, int MODEL, class SH, unsigned FORM = 0u>
__device__ __forceinline__ void pc_consume(const RolloutArgs& A, const SH& sh, double& cost, const int b, const int lane,
                                           int* prune_on = nullptr,   // wave-uniform switch of the window pruning (below)
                                           const ObstLds* ob = kNoDiscs, const ObstMovLds* obm = kNoDiscs,   // kDiscs / kMovingDiscs
                                           int* taken_flag = nullptr, const int taken_value = 0) {   // see below
    constexpr bool LEAN = (FORM & kLeanRegisters) != 0, OBST = (FORM & kDiscs) != 0, MOVING = (FORM & kMovingDiscs) != 0;
    static_assert(!MOVING || OBST, "moving discs are discs");
    const int H4 = (A.H + 3) & ~3;   // the window is padded with c = +inf: four points per iteration, no remainder
    double px[NV], py[NV], m[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        px[i] = sh.p[b & (SH::kPBuf - 1)][i][0][lane];
        py[i] = sh.p[b & (SH::kPBuf - 1)][i][1][lane];
        if constexpr (SH::kStage) {   // staged positions are absolute
            px[i] -= A.x0[0];
            py[i] -= A.x0[1];
        }
        m[i] = INFINITY;
    }
    if (taken_flag) {
        // three-wave kernel: the positions of the block are in registers -- tell the producer that the LDS buffer is free
        // (mppi_rollout_r3.h).  The wait makes sure the loads above have returned before the number is written.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pc_publish(taken_flag, taken_value);
    }
    // software pipeline: the coefficients of points j+4..j+7 are read from LDS (broadcast reads) before the ~100 fp64
    // instructions on points j..j+3 issue, so no iteration waits out the LDS latency.  sh.ab / sh.c carry 4 spare
    // entries past H4, so the last iteration's read-ahead stays inside the arrays.
    double2 ab0[4], ab1[4];
    double c0[4], c1[4];
    auto fetch = [&](double2(&ab)[4], double(&c)[4], const int j) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            ab[jj] = sh.ab[j + jj];
            c[jj] = sh.c[j + jj];
        }
    };
    auto points4 = [&](const double2(&ab)[4], const double(&c)[4]) {
        double f[4][NV];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int i = 0; i < NV; ++i) f[jj][i] = fma(ab[jj].x, px[i], fma(ab[jj].y, py[i], c[jj]));
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            // the three minima over freshly computed values need no canonicalising v_max; the loop-carried one would get
            // one per iteration from the compiler (it cannot see through the phi that m is already quiet), so it is
            // issued directly: v_min_f64 of two quiet operands
            const double t = fmin(fmin(f[0][i], f[1][i]), fmin(f[2][i], f[3][i]));
            asm("v_min_f64 %0, %1, %2" : "=v"(m[i]) : "v"(m[i]), "v"(t));
        }
    };
    // ---- exact pruning of the window (pc_prune_window above): the loop runs over the hull [jb, je) of the window points
    // that can be the nearest one for some sample of this wave
    int jb = 0, je = H4;
    if (A.prune && (prune_on == nullptr || *prune_on)) {
        if (H4 > 64) pc_prune_window<NV, 2>(A, sh, px, py, lane, jb, je);
        else pc_prune_window<NV, 1>(A, sh, px, py, lane, jb, je);
        // the samples of a wave fan out with time: once a block keeps more than 3/4 of the window the later ones will too,
        // and the wave stops testing for the rest of the launch
        if (prune_on && 4 * (je - jb) > 3 * H4) *prune_on = 0;
    }
    if constexpr (LEAN) {
        double2 qa[2], qb[2];
        double ca[2], cb[2];
        auto fetch2 = [&](double2(&ab)[2], double(&c)[2], const int j) {
            ab[0] = sh.ab[j];
            c[0] = sh.c[j];
            ab[1] = sh.ab[j + 1];
            c[1] = sh.c[j + 1];
        };
        auto points2 = [&](const double2(&ab)[2], const double(&c)[2]) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double f0 = fma(ab[0].x, px[i], fma(ab[0].y, py[i], c[0]));
                const double f1 = fma(ab[1].x, px[i], fma(ab[1].y, py[i], c[1]));
                const double t = fmin(f0, f1);
                asm("v_min_f64 %0, %1, %2" : "=v"(m[i]) : "v"(m[i]), "v"(t));
            }
        };
        // the first pair of points starts the minimum (no +inf to initialise, no minimum against it: the hull is never empty,
        // je - jb is a multiple of 4, and min(+inf, t) = t for every t the loop can produce but NaN, which ends at the gate
        // value either way); the read-ahead ends inside the arrays' padding
        auto first2 = [&](const double2(&ab)[2], const double(&c)[2]) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const double f0 = fma(ab[0].x, px[i], fma(ab[0].y, py[i], c[0]));
                const double f1 = fma(ab[1].x, px[i], fma(ab[1].y, py[i], c[1]));
                m[i] = fmin(f0, f1);
            }
        };
        fetch2(qa, ca, jb);
        fetch2(qb, cb, jb + 2);
        __builtin_amdgcn_sched_barrier(0);
        first2(qa, ca);
        fetch2(qa, ca, jb + 4);
        __builtin_amdgcn_sched_barrier(0);
        points2(qb, cb);
        for (int j = jb + 4; j < je; j += 4) {
            fetch2(qb, cb, j + 2);
            __builtin_amdgcn_sched_barrier(0);
            points2(qa, ca);
            fetch2(qa, ca, j + 4);
            __builtin_amdgcn_sched_barrier(0);
            points2(qb, cb);
        }
    } else {
    fetch(ab0, c0, jb);
    for (int j = jb; j < je; j += 8) {   // two register sets in ping-pong: no copies
        fetch(ab1, c1, j + 4);
        __builtin_amdgcn_sched_barrier(0);   // keep the read-ahead above the arithmetic (the scheduler would sink it)
        points4(ab0, c0);
        if (j + 4 >= je) break;
        fetch(ab0, c0, j + 8);
        __builtin_amdgcn_sched_barrier(0);
        points4(ab1, c1);
    }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        // d^2 = |p|^2 + min_j(...), gate d <= 100 (dd:185), cost += path_weight*d*d (dd:206)
        double d2 = m[i] + fma(px[i], px[i], py[i] * py[i]);
        if constexpr (MODEL == CCV_MPPI_FULL_BODY) {   // (kept as it was: the one-wave full-body kernel is at its register limit)
            d2 = d2 < 1.0e4 ? fmax(d2, 0.0) : 1.0e4;   // NaN -> gate value, as `distance < min_distance` (dd:189) is false for NaN
            cost += A.w_path * d2;
        } else {
            // the same value in two instructions instead of four (compare, max, two selects): min(d2, 1e4) first -- of a NaN
            // and a number v_min_f64 returns the number (d2 is the result of arithmetic: never a signalling NaN), which is
            // the gate value -- then max(., 0); and the weight rides on the addition
            double g;
            asm("v_min_f64 %0, %1, %2" : "=v"(g) : "v"(d2), "s"(1.0e4));
            asm("v_max_f64 %0, %1, 0" : "=v"(d2) : "v"(g));
            cost = fma(A.w_path, d2, cost);
        }
    }
    if constexpr (MOVING) obst_term_moving<NV>(A, *obm, px, py, m, cost, b * kTU);
    else if constexpr (OBST) obst_term<NV>(A, *ob, px, py, m, cost);
}

// pc_consume for a block of which nv states reach the path cost (wave-uniform; none: nothing happens, the caller's hand-off
// included).  A switch: written as a chain of comparisons, the same dispatch changed every one-wave kernel's instructions.
template <int MODEL, class SH, unsigned FORM = 0u>
__device__ __forceinline__ void pc_consume_states(const int nv, const RolloutArgs& A, const SH& sh, double& cost, const int b, const int lane,
                                                  int* prune_on, const ObstLds* ob = kNoDiscs, const ObstMovLds* obm = kNoDiscs,
                                                  int* taken_flag = nullptr, const int taken_value = 0) {
    switch (nv) {
        case 8: pc_consume<8, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 7: pc_consume<7, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 6: pc_consume<6, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 5: pc_consume<5, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 4: pc_consume<4, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 3: pc_consume<3, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 2: pc_consume<2, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        case 1: pc_consume<1, MODEL, SH, FORM>(A, sh, cost, b, lane, prune_on, ob, obm, taken_flag, taken_value); break;
        default: break;
    }
}

}  // namespace ccv

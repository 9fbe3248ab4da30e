// Small device helpers every kernel header may use: compile-time loops, the uniform-divisor quotient, the clamp forms, wave-
// uniform values and the DPP cross-lane reductions.  Nothing here knows a kernel argument.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace ccv {

template <int N, class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl<N>(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// x / d for a wave-uniform divisor d whose reciprocal r = RN(1 / d) was formed once: q = RN(x r), the exact remainder
// x - q d by FMA, one correction -- the correctly rounded quotient (Markstein's theorem for a faithful q and a correctly
// rounded r), in 3 instructions instead of the ~10 of an fp64 division.  The full-body ZMP term divides by dt twice per
// sample-step (fb:469, fb:479-481).  (Its third division, by mass * gravity_.z (fb:601), stays a division: one more pair of
// kernel-argument registers pushes the one-wave full-body kernel from 232 to 256 VGPRs with 17 spilled -- SGPR spills live
// in VGPR lanes -- and costs more than the division: C4 287 -> 294 us, measured.)  Valid while nothing overflows or
// vanishes on the way (the host admits the kernels that use it only for 1e-100 <= |dt| <= 1e100 and control bounds below
// 1e100, fast_trig_safe(); anything else runs the plain kernel with true divisions); a zero quotient may lose its sign.
__device__ __forceinline__ double div_uniform(const double x, const double d, const double r) {
    const double q = x * r;
    return fma(fma(-q, d, x), r, q);
}

// dd:62-67
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// The same value in two instructions instead of six (two compares, four selects) -- for every v that is not NaN and bounds
// with lo <= hi (NaN bounds pass v through in both forms).  The reference's clamp passes a NaN control through (dd:98-99: both
// comparisons are false), min / max would replace it by a bound: the kernels use this form only where the host has checked
// sigma and the bounds and the kernel itself has found no NaN in the warm start (RolloutArgs::fast_clamp; a control is
// double(z) * sigma + u* with a finite z).  (-0 against a bound of +0 comes out as +0 here and -0 there: equal values.)
// Where the other form lives: the one-wave kernel chooses per block; the four-wave kernel (mppi_rollout_r4.h) has, for diff
// drive and steering, one loop over the time blocks per form and chooses the loop -- the compare-and-select form costs a launch
// that does not need it no register and no instruction; full body keeps the choice in its loop.
__device__ __forceinline__ double clampd_fast(double v, double lo, double hi) { return __builtin_fmin(__builtin_fmax(v, lo), hi); }
template <bool FAST>
__device__ __forceinline__ double clampd_as(double v, double lo, double hi) {
    if constexpr (FAST) return clampd_fast(v, lo, hi);
    else return clampd(v, lo, hi);
}

// a wave-uniform double into scalar registers (the compiler cannot see that a converted integer is uniform)
__device__ __forceinline__ double uniform_f64(const double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// ---- cross-lane reductions (DPP) ---------------------------------------------------------------------------------

// Cross-lane moves of an fp64 value as two DPP moves (ALU latency) instead of ds_bpermute (an LDS round trip, ~250
// cycles per butterfly step with its wait): a 64-lane reduction drops from ~1500 to ~150 cycles.
template <int CTRL>
__device__ __forceinline__ double dpp_move(const double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]: lane ^ 1
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]: lane ^ 2
constexpr int kDppHalfMirror = 0x141;   // row_half_mirror: lane i <-> 7 - i within 8
constexpr int kDppMirror = 0x140;       // row_mirror: lane i <-> 15 - i within 16

__device__ __forceinline__ double lane_value(const double v, const int lane) {   // wave-uniform result
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Fixed-shape reductions over the 64 lanes (every lane of a 16-lane row ends with the row's result; the four rows are
// combined as (r0 op r1) op (r2 op r3)); the result is wave-uniform.
#define CCV_WAVE_REDUCE(name, OP)                                                         \
    __device__ __forceinline__ double name(double v) {                                    \
        v = OP(v, dpp_move<kDppXor1>(v));                                                 \
        v = OP(v, dpp_move<kDppXor2>(v));                                                 \
        v = OP(v, dpp_move<kDppHalfMirror>(v));                                           \
        v = OP(v, dpp_move<kDppMirror>(v));                                               \
        return OP(OP(lane_value(v, 0), lane_value(v, 16)), OP(lane_value(v, 32), lane_value(v, 48))); \
    }
__device__ __forceinline__ double op_add(const double a, const double b) { return a + b; }
__device__ __forceinline__ double op_min(const double a, const double b) { return fmin(a, b); }
__device__ __forceinline__ double op_max(const double a, const double b) { return fmax(a, b); }
CCV_WAVE_REDUCE(wave_sum, op_add)
CCV_WAVE_REDUCE(wave_min, op_min)
CCV_WAVE_REDUCE(wave_max, op_max)
#undef CCV_WAVE_REDUCE

// Four 64-lane fp32 reductions at once, each one DPP-modified VALU instruction per step (the compiler does not fold a DPP
// move into v_min / v_max and puts a canonicalising v_max in front of every fminf): 24 instructions + 4 v_readlane for
// four results, against ~25 per fp64 reduction above.  The four chains are interleaved, so a step's DPP read of a register
// is four instructions behind its write (the DPP hazard needs two wait states; the leading s_nop covers the producer of
// the inputs, which the compiler's hazard recogniser cannot see into from outside the asm).  row_bcast:15 / :31 carry a
// row's result into the next row(s); lane 63 ends with the result of all 64 lanes.  NaN operands are ignored (IEEE
// minNum / maxNum); all 64 lanes must be active.
#define CCV_RED4_STEP(O0, O1, O2, O3, CTRL)                                                           \
    O0 " %0, %0, %0 " CTRL "\n\t" O1 " %1, %1, %1 " CTRL "\n\t" O2 " %2, %2, %2 " CTRL "\n\t" O3 " %3, %3, %3 " CTRL "\n\t"
#define CCV_RED4(NAME, O0, O1, O2, O3)                                                                \
    __device__ __forceinline__ void NAME(float& a, float& b, float& c, float& d) {                    \
        asm volatile("s_nop 1\n\t"                                                                    \
                     CCV_RED4_STEP(O0, O1, O2, O3, "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")  \
                     CCV_RED4_STEP(O0, O1, O2, O3, "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")  \
                     CCV_RED4_STEP(O0, O1, O2, O3, "row_half_mirror row_mask:0xf bank_mask:0xf")      \
                     CCV_RED4_STEP(O0, O1, O2, O3, "row_mirror row_mask:0xf bank_mask:0xf")           \
                     CCV_RED4_STEP(O0, O1, O2, O3, "row_bcast:15 row_mask:0xa bank_mask:0xf")         \
                     CCV_RED4_STEP(O0, O1, O2, O3, "row_bcast:31 row_mask:0xc bank_mask:0xf")         \
                     : "+v"(a), "+v"(b), "+v"(c), "+v"(d));                                           \
        a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 63));                         \
        b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 63));                         \
        c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), 63));                         \
        d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 63));                         \
    }
CCV_RED4(wave_min_max_min_max_f32, "v_min_f32_dpp", "v_max_f32_dpp", "v_min_f32_dpp", "v_max_f32_dpp")
CCV_RED4(wave_min4_f32, "v_min_f32_dpp", "v_min_f32_dpp", "v_min_f32_dpp", "v_min_f32_dpp")
#undef CCV_RED4
#undef CCV_RED4_STEP

}  // namespace ccv

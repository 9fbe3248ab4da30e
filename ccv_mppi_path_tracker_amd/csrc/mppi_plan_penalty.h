// The traversal multiplier of a free cell in a weighted plan (mppi_plan_cost.h has the statement): one fp32
// multiplication, a clamp and a truncation.  Floats and integers only, so that the kernel (k_plan_cost.hip) and a stand-alone host
// program (tools/plan_penalty_check.cpp) run the same lines.  Built without contraction, as everything here.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CCV_PLAN_HD __host__ __device__
#else
#define CCV_PLAN_HD
#endif

namespace ccv {

constexpr int kPlanMaxPenalty = 15;   // CCV_MPPI_PLAN_MAX_PENALTY

// m(c) = 1 + q(c), 1 .. 1 + max_penalty: q = 0 where !(t > 0) (a cell or a product that is zero, negative or NaN), max_penalty
// where t >= max_penalty (an infinite product too), else t truncated.  max_penalty in [0, kPlanMaxPenalty].
CCV_PLAN_HD inline uint32_t plan_multiplier(const float cell, const float gain, const int32_t max_penalty) {
    const float t = cell * gain;
    if (!(t > 0.0f)) return 1u;
    if (t >= (float)max_penalty) return 1u + (uint32_t)max_penalty;
    return 1u + (uint32_t)(int32_t)t;
}

}  // namespace ccv

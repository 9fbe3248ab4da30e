// Paths planned on the device with traversal weights from the cell costs (ccv_mppi_batch_resident_set_plan_penalty; DESIGN.md
// section 10t).  All of mppi_plan.h stands -- blocked, the eight moves, no corner cutting, the uint16 field, the start cell, the
// status order, the pose formula -- and every free cell gets a multiplier from two handle-wide values, gain and max_penalty:
//     t = cell(c) * gain                    (one fp32 multiplication, no FMA)
//     q(c) = !(t > 0) ? 0 : (t >= (float)max_penalty ? max_penalty : (int)t)         (mppi_plan_penalty.h)
//     m(c) = 1 + q(c)
//     step(c -> n) = w(c, n) * m(c)         w = 5 straight, 7 diagonal: the cell that is LEFT is charged
//     field      the one fixpoint of D(c) = min(D(c), min(kPlanFar, D(n) + step(c -> n))), D(goal) = 0
//     descent    the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with D(n) + step(c -> n) == D(c)
// The rule is not symmetric: D is the charge TO the goal.  A relaxation of c needs one multiplier, its own.  The kernel is
// k_plan_cost.hip's, a unit of its own: k_plan.hip's kernel is launched while every multiplier is 1 (capi_batch_plan.hip).
#pragma once
#include "mppi_plan.h"
#include "mppi_plan_penalty.h"

namespace ccv {

// One launch for the n entries of a call; gain finite and > 0, max_penalty in [1, kPlanMaxPenalty].
void launch_plan_field_cost(const PlanEntry* entries, int32_t n, float lethal, int32_t max_sweeps, float gain, int32_t max_penalty, hipStream_t stream);

}  // namespace ccv

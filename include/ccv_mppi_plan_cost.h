/*
 * ccv_mppi_plan_cost.h -- traversal weights for the paths planned on the device in the batch handles' device-resident closed
 * loop (libccv_mppi_hip.so).
 *
 * An extension of ccv_mppi.h with the conventions of that header; ccv_mppi.h includes this file, so either include gives the
 * two calls.  What they promise is written once, in ccv_mppi.h ("Paths planned on the device: traversal weights"); the six calls
 * of ccv_mppi_plan.h and the five that run the resident loop itself stay where they are: a caller whose plans weigh every free
 * cell alike needs nothing from here.  The rule in short: a step out of cell c costs w * (1 + q(c)), w = 5 straight, 7 diagonal,
 *     t = cell(c) * gain;   q(c) = !(t > 0) ? 0 : (t >= (float)max_penalty ? max_penalty : (int)t)
 */
#ifndef CCV_MPPI_PLAN_COST_H_
#define CCV_MPPI_PLAN_COST_H_

#include "ccv_mppi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CCV_MPPI_PLAN_MAX_PENALTY 15 /* max_penalty at most: a multiplier is 1..16 */

/* _set_plan_penalty: after _resident_set_plan; host state only; (0, 0): every multiplier is 1, the plan of ccv_mppi_plan.h.
 * _get_plan_penalty: either pointer may be NULL. */
int ccv_mppi_batch_resident_set_plan_penalty(ccv_mppi_batch* b, float gain, int32_t max_penalty);
int ccv_mppi_batch_resident_get_plan_penalty(ccv_mppi_batch* b, float* gain, int32_t* max_penalty);

#ifdef __cplusplus
}
#endif
#endif /* CCV_MPPI_PLAN_COST_H_ */

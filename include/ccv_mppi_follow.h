/*
 * ccv_mppi_follow.h -- costmaps that follow their robots in the batch handles' device-resident closed loop (libccv_mppi_hip.so).
 *
 * An extension of ccv_mppi.h with the conventions of that header; ccv_mppi.h includes this file, so either include gives the
 * five calls.  What they promise is written once, in ccv_mppi.h ("Costmaps that follow their robots"); the five calls that run
 * the resident loop itself stay alone in ccv_mppi.h, as with ccv_mppi_fleet.h, ccv_mppi_sense.h and ccv_mppi_plan.h: a caller
 * whose maps stay where they are needs nothing from here.  The decision in short, per axis and each axis on its own:
 *     e = floor((pose - origin) * inv) - n / 2;   d = |e| <= margin ? 0 : clamp(e, -max_step, max_step)
 */
#ifndef CCV_MPPI_FOLLOW_H_
#define CCV_MPPI_FOLLOW_H_

#include "ccv_mppi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a map's last follow call (0: the map has never been followed) */
#define CCV_MPPI_FOLLOW_MOVED 1
#define CCV_MPPI_FOLLOW_HELD 2
#define CCV_MPPI_FOLLOW_NO_POSE 3
#define CCV_MPPI_FOLLOW_LIMIT 4

/* _set_follow: a setter, after _set_occupancy; on = 0: following off.  _follow_enqueue: stream-ordered, two kernel launches.
 * _read_follow synchronises.  _plan_goals_enqueue: _plan_enqueue (ccv_mppi_plan.h) with world goals. */
int ccv_mppi_batch_resident_set_follow(ccv_mppi_batch* b, int32_t on);
int ccv_mppi_batch_resident_get_follow(ccv_mppi_batch* b, int32_t* on);
int ccv_mppi_batch_resident_follow_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* instance /*[n]*/, int32_t margin, int32_t max_step,
                                           int32_t fill);
int ccv_mppi_batch_resident_read_follow(ccv_mppi_batch* b, int32_t* status /*[n_maps]*/, int32_t* shift /*[n_maps][2]*/,
                                        int64_t* offset /*[n_maps][2]*/, double* origin /*[n_maps][2]*/);
int ccv_mppi_batch_resident_plan_goals_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* instance /*[n]*/, const double* goal_xy /*[n][2]*/,
                                               float lethal, int32_t max_sweeps);

#ifdef __cplusplus
}
#endif
#endif /* CCV_MPPI_FOLLOW_H_ */

/*
 * ccv_mppi_plan.h -- paths planned on the device for the batch handles' device-resident closed loop (libccv_mppi_hip.so).
 *
 * An extension of ccv_mppi.h with the conventions of that header; ccv_mppi.h includes this file, so either include gives the
 * six calls.  What they promise is written once, in ccv_mppi.h ("Paths planned on the device"); the five calls that run the
 * resident loop itself stay alone in ccv_mppi.h, as with ccv_mppi_fleet.h and ccv_mppi_sense.h: a caller that never plans needs
 * nothing from here.  Diagonal poses of a planned path are sqrt(2) * resolution apart, straight ones resolution.
 */
#ifndef CCV_MPPI_PLAN_H_
#define CCV_MPPI_PLAN_H_

#include "ccv_mppi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CCV_MPPI_PLAN_MAX_FIELD 81920 /* (nx + 2)(ny + 2) of a map that is planned on: the field and a border, uint16, in LDS */
#define CCV_MPPI_PLAN_MAX_POSES 16384 /* capacity of one instance */
/* status of an instance's last plan (0: it has never planned) */
#define CCV_MPPI_PLAN_OK 1
#define CCV_MPPI_PLAN_TRUNCATED 2
#define CCV_MPPI_PLAN_NO_START 3
#define CCV_MPPI_PLAN_START_BLOCKED 4
#define CCV_MPPI_PLAN_GOAL_BLOCKED 5
#define CCV_MPPI_PLAN_UNREACHABLE 6
#define CCV_MPPI_PLAN_NOT_CONVERGED 7

/* _set_plan: a setter, after _resident_set_paths; capacity NULL: planning off.  _plan_enqueue: stream-ordered, one kernel launch.
 * The three _read_ calls synchronise. */
int ccv_mppi_batch_resident_set_plan(ccv_mppi_batch* b, const int32_t* capacity /*[B], 0..MAX_POSES*/, int32_t keep_fields);
int ccv_mppi_batch_resident_get_plan(ccv_mppi_batch* b, int32_t* capacity, int32_t* keep_fields);
int ccv_mppi_batch_resident_plan_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* instance /*[n]*/, const int32_t* goal_xy /*[n][2]*/,
                                         float lethal, int32_t max_sweeps);
int ccv_mppi_batch_resident_read_plan(ccv_mppi_batch* b, int32_t* status, int32_t* poses /*L or 0*/, int32_t* start_cell /*[B][2]*/,
                                      int32_t* start_dist /*D(s) or -1*/, int32_t* sweeps);
int ccv_mppi_batch_resident_read_plan_field(ccv_mppi_batch* b, int32_t instance, uint16_t* out /*[ny][nx]*/);
int ccv_mppi_batch_resident_read_path(ccv_mppi_batch* b, int32_t instance, int32_t max_poses, double* x, double* y, int32_t* n_path);

#ifdef __cplusplus
}
#endif
#endif /* CCV_MPPI_PLAN_H_ */

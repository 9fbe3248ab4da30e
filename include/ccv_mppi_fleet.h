/*
 * ccv_mppi_fleet.h -- the fleet term of the batch handles' device-resident closed loop (libccv_mppi_hip.so).
 *
 * An extension of ccv_mppi.h with the conventions of that header; ccv_mppi.h includes this file, so either include gives
 * the three calls.  The five calls that run the resident loop itself (ccv_mppi_batch_resident_set_paths ... _read_trace)
 * stay in ccv_mppi.h: a caller that never turns the term on needs nothing from here.
 */
#ifndef CCV_MPPI_FLEET_H_
#define CCV_MPPI_FLEET_H_

#include "ccv_mppi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fleet term: the robots of one resident batch keep clear of each other (NOT reference behaviour; off by default; resident
 * steps only).  While it is on, every resident tick gives instance y a disc list of two parts: its n_static[y] discs of
 * ccv_mppi_batch_set_obstacles, unchanged, then up to M_y = min(max_neighbours, CCV_MPPI_MAX_OBSTACLES - n_static[y]) discs for
 * the nearest other robots: centre q_j, radius radius[y] + radius[j].  The obstacle term of _set_obstacles charges them with
 * weight[y].  Every position of a tick is the pose at the start of that tick, before its advance (the own one too): a
 * neighbour's disc stands where that robot was one tick ago, and the caller covers its motion of one period with the radius --
 * or turns on ccv_mppi_batch_set_fleet_prediction (ccv_mppi.h), with which the disc moves over the horizon at the velocity the
 * robot had over its last tick.
 * Selection, all in fp64 without FMA: dx = q_j[0] - q_y[0], dy = q_j[1] - q_y[1], d2 = dx*dx + dy*dy; robot j != y is a
 * candidate iff d2 <= range*range (the product rounded once; a NaN fails); the candidates in (d2, j) order, the first M_y taken
 * and written in that order.  The lists are formed on the device in the prologue of the tick, with no host data and no
 * synchronisation.
 * radius, weight: [B], finite and >= 0; range: finite and >= 0; 1 <= max_neighbours <= CCV_MPPI_MAX_OBSTACLES; at most 1024
 * instances; otherwise CCV_MPPI_ERR_INVALID_ARG and nothing changes.  Flushes a pending resident update and synchronises, like
 * _set_obstacles; a handle without _set_params gets B copies of its configuration in the parameter table.  There is one weight
 * per instance: the later of _set_fleet and _set_obstacles sets it, and both getters return it.  While the term is on:
 * _last_kernel carries CCV_MPPI_BATCH_KERNEL_OBST; _set_obstacles changes the static rows and counts only, and
 * _set_obstacles(NULL) removes the static discs and keeps weights and fleet; _set_params keeps discs and fleet;
 * ccv_mppi_batch_iterate and _iterate_enqueue return CCV_MPPI_ERR_STATE and launch nothing (the lists exist only where the
 * poses live).  radius == NULL with max_neighbours == 0 turns the term off; with no static discs the handle returns to the
 * kernels, and the bits, that ran before.
 * _get_fleet: radius [B] (zeros while off), range, max_neighbours (0 while off); any pointer may be NULL.
 * _read_fleet: synchronises; the lists the last tick's rollout was charged with (after a setter and before the next tick: the
 * static part alone): n_static [B], n_total [B], xyr [B][CCV_MPPI_MAX_OBSTACLES][3] with the rows past n_total zero; any
 * pointer may be NULL; CCV_MPPI_ERR_STATE while the term is off. */
int ccv_mppi_batch_resident_set_fleet(ccv_mppi_batch* b, const double* radius, double range, int32_t max_neighbours,
                                      const double* weight);
int ccv_mppi_batch_resident_get_fleet(ccv_mppi_batch* b, double* radius, double* range, int32_t* max_neighbours);
int ccv_mppi_batch_resident_read_fleet(ccv_mppi_batch* b, int32_t* n_static, int32_t* n_total, double* xyr);

#ifdef __cplusplus
}
#endif
#endif /* CCV_MPPI_FLEET_H_ */

/*
 * ccv_mppi_sense.h -- the simulated range sensor of the batch handles' device-resident closed loop (libccv_mppi_hip.so).
 *
 * An extension of ccv_mppi.h with the conventions of that header; ccv_mppi.h includes this file, so either include gives the
 * two calls.  What they promise is written once, in ccv_mppi.h beside ccv_mppi_batch_set_world ("Range sensors simulated on the
 * device"), with the world's own four calls; the five calls that run the resident loop itself stay alone in ccv_mppi.h, as with
 * ccv_mppi_fleet.h: a caller that never senses needs nothing from here.
 */
#ifndef CCV_MPPI_SENSE_H_
#define CCV_MPPI_SENSE_H_

#include "ccv_mppi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* _resident_sense_enqueue: the n named instances cast the beams beam_xy [n_beams][2] through the world of
 * ccv_mppi_batch_set_world from their resident poses, into their own costmaps; stream-ordered, two kernel launches.
 * _resident_read_sense: first [B][max_beams] and sensor_cell [B][2] of every instance's last sensing; synchronises. */
int ccv_mppi_batch_resident_sense_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* instance /*[n]*/, int32_t n_beams,
                                          const int32_t* beam_xy /*[n_beams][2]*/, int32_t clear_value, int32_t mark_value);
int ccv_mppi_batch_resident_read_sense(ccv_mppi_batch* b, int32_t* first /*[B][max_beams]*/, int32_t* sensor_cell /*[B][2]*/);

#ifdef __cplusplus
}
#endif
#endif /* CCV_MPPI_SENSE_H_ */

// Range sensors simulated on the device (ccv_mppi_batch_resident_sense_enqueue): every named robot of a
// resident batch casts one shared table of beams through a ground-truth world map from the cell its own resident pose lies in,
// and the result goes into the robot's costmap.  Integers only after one pose-to-cell step:
//     fx = (x - origin_x) * inv,  fy likewise     (the world's origin; inv = RN(1 / resolution), the host's; no FMA)
//     in = fx >= 0 && fx < nx && fy >= 0 && fy < ny;  s = ((int)fx, (int)fy)       (not in: the robot senses nothing)
//     beam (dx, dy): the cells i = 0 .. a of mppi_costmap_scan.h's line from s to s + (dx, dy) (cell a is the end cell)
//     f = min { i in [1, a] : cell i inside the world and world[cell i] >= threshold }
//     local cell = world cell - (off_x, off_y)    (the anchor plus the cells the map has rolled)
//     f exists: the local cells of i in [0, f) = clear_value, local cell f = mark_value;  else the local cells of i in [0, a) = clear_value
// -- local cells outside the map skipped, marks after ALL clears of the map.  first[r] = f or -1.  The float cells follow in the
// next launch: launch_inflate_rects (mppi_costmap.h) over the table this kernel writes, one rectangle per entry -- the box
// s_local + [min dx, max dx] x [min dy, max dy] clipped to the map, grown by R and clipped again (grown_rect's arithmetic,
// mppi_costmap_rects.h), empty for a robot that senses nothing.  The kernel is k_costmap_sense.hip's; the entries and the beams
// live in the staging slot of the call (pinned host memory, read in place), the world, `first`, the sensor cells and the
// rectangle table in device memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mppi_costmap.h"

namespace ccv {

constexpr int kSenseMaxBeams = 4096;   // CCV_MPPI_SENSE_MAX_BEAMS

// One sensing robot.  All writes to its map come from the one workgroup of its entry.
struct alignas(16) SenseEntry {
    InflateArgs rect;       // the map's inflation, complete but for x0, y0, w, h: the kernel forms those and writes the table's row
    uint8_t* layer;         // [ny][nx] front (rect.layer, writable)
    const double* pose;     // the robot's resident pose: x, y
    int32_t* first;         // [n_beams] the robot's row of the read-back
    int32_t* sensor_cell;   // [2] ... and its world cell
    int32_t off_x, off_y;   // the world cell of the map's cell (0, 0) now
    int32_t pad[2];
};
static_assert(sizeof(SenseEntry) == 112, "a table of the staging slot");

// What the entries of a call share; travels in the kernel-argument segment.
struct SenseArgs {
    const uint8_t* world;     // [wny][wnx]
    const int32_t* beam_xy;   // [n_beams][2] end offsets
    double origin_x, origin_y, inv;
    int32_t wnx, wny, threshold, n_beams;
    int32_t min_dx, max_dx, min_dy, max_dy;   // the extent of the beam table and the offset (0, 0)
    int32_t clear_value, mark_value;
};

// One launch for the n entries of a call; rects [n]: the table launch_inflate_rects reads next.
void launch_sense_trace(const SenseEntry* entries, InflateArgs* rects, int32_t n, const SenseArgs& args, hipStream_t stream);

}  // namespace ccv

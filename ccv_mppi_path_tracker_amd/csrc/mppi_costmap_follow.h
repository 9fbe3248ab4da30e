// Costmaps that follow their robots (ccv_mppi_batch_resident_follow_enqueue): the window of a
// device-inflated costmap (mppi_costmap.h) is re-centred on the resident pose of its robot, decided on the device.  For a named
// instance with map m, the map's frame as the stream finds it (cx, cy, origin_x, origin_y) and the resident pose (x, y):
//     fx = (x - origin_x) * inv,  fy likewise     (the grid term's formula: inv = RN(1 / resolution), the host's; no FMA)
//     ok = fabs(fx) < 2^30 && fabs(fy) < 2^30     (false for a NaN or infinite pose)
//     px = (int64)floor(fx), py likewise          (floor: the pose may lie left of or below the map)
//     ex = px - nx / 2,  ey = py - ny / 2         (C integer division: the centre cell)
//     dx = |ex| <= margin ? 0 : clamp(ex, -max_step, max_step),  dy likewise, each axis on its own
//     cx' = cx + dx, cy' = cy + dy;  |cx'| > 2^30 or |cy'| > 2^30, or a rolled origin not finite: nothing moves
//     origin' = origin0 + (double)cx' * resolution     (one multiplication, one addition, no FMA: the host roll's formula)
//     status: 1 MOVED, 2 HELD (dx = dy = 0), 3 NO_POSE (!ok), 4 LIMIT; 0: the map has never been followed
// follow_decide (mppi_costmap_follow_decide.h) is that statement, for the device and for a stand-alone host program.
// Two launches for all entries of a call: k_follow_shift decides, writes the back layer and the back float cells from the front
// ones (a roll by (dx, dy) with every exposed cell `fill`, or a plain copy where nothing moves: the host cannot know which, so
// every named map changes buffers), the other slot of the map's frame, the instances' grid rows, the result row and four band
// rectangles (roll_bands, mppi_costmap_rects.h; empty ones w = h = 0) in a device table; launch_inflate_rects (mppi_costmap.h)
// derives the float cells of those bands again.  A map has two frame slots; the host knows how often the map was followed and
// with that which slot is current: every workgroup of an entry reads the current slot, which no workgroup writes, and arrives at
// the same decision.  The kernel is k_costmap_follow.hip's; the entries live in the staging slot of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mppi_costmap.h"
#include "mppi_costmap_follow_decide.h"
#include "mppi_costmap_sense.h"
#include "mppi_kernels.h"
#include "mppi_plan.h"

namespace ccv {

// One following robot.  Every workgroup of the entry decides for itself from `pose` and `frame_src`; the first one writes
// frame_dst, the result row, the rectangles and the grid rows.
struct alignas(16) FollowEntry {
    InflateArgs rect;              // the map's inflation over the back buffers, complete but for x0, y0, w, h
    const uint8_t* layer_src;      // [ny][nx] front
    uint8_t* layer_dst;            // [ny][nx] back
    const float* cells_src;        // [ny][nx] front: the grid rows that point here are the map's
    float* cells_dst;              // [ny][nx] back
    const double* pose;            // the robot's resident pose: x, y
    const FollowFrame* frame_src;  // the map's current slot
    FollowFrame* frame_dst;        // ... and the other one
    int32_t* result;               // [kFollowResultInts]
    double ox0, oy0, resolution, inv;
    int32_t nx, ny, margin, max_step, fill, pad[3];
};
static_assert(sizeof(FollowEntry) == 192, "a table of the staging slot");

// Launch 1: n entries, rects [n][kFollowRects] in device memory, the grid rows [B] of the handle.  (Launch 2: launch_inflate_rects
// over rects.)
void launch_follow_shift(const FollowEntry* entries, InflateArgs* rects, int32_t n, int64_t max_cells, GridRow* rows, int32_t B, hipStream_t stream);

// The consumers in the frame only the device knows.  k_sense_trace (mppi_costmap_sense.h) and k_plan_field (mppi_plan.h) stay as
// they are and read tables of their own entries; while the maps follow, those tables live in device memory and one small launch
// ahead of the kernel completes them from the maps' current frame slots (a followed form over a shared inlined body compiles the
// unfollowed kernels to other instructions: DESIGN.md section 10s).
// Sensing: entry.off_x, off_y hold the anchor alone; the rolled count (cx, cy) is added here (|anchor| <= 2^29, |cx| <= 2^30:
// the sum is an int32).
struct alignas(16) SenseFollowEntry {
    SenseEntry entry;
    const FollowFrame* frame;
    int64_t pad;
};
static_assert(sizeof(SenseFollowEntry) == 128, "a table of the staging slot");
// Planning: the origin is the frame slot's; with world_goal the goal is the world point (goal_wx, goal_wy), turned into a cell
// here against that origin and clamped to the map (f < 0 or NaN -> 0, f >= n -> n - 1, else (int)f: batch.goal_cells' arithmetic,
// one subtraction, one multiplication).
struct alignas(16) PlanFollowEntry {
    PlanEntry entry;
    const FollowFrame* frame;
    double goal_wx, goal_wy;
    int32_t world_goal, pad;
};
static_assert(sizeof(PlanFollowEntry) == 160, "a table of the staging slot");
void launch_follow_resolve_sense(const SenseFollowEntry* in, SenseEntry* out, int32_t n, hipStream_t stream);
void launch_follow_resolve_plan(const PlanFollowEntry* in, PlanEntry* out, int32_t n, hipStream_t stream);

}  // namespace ccv

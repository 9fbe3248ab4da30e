// Rolling costmaps (ccv_mppi_batch_roll_occupancy_enqueue): the window of a device-inflated costmap
// (mppi_costmap.h) moves by whole cells.  With `old` and `new` the layer before and after a roll by (dx, dy):
//     new(ix, iy) = old(ix + dx, iy + dy)      where (ix + dx, iy + dy) lies inside the map
//                 = the caller's cell, or fill elsewhere (the exposed cells)
// and the float cells are the transform of mppi_costmap.h over `new`, complete.  Two launches for all maps of a call:
// k_roll_shift writes the back layer and the back float cells from the front ones and points the instances' grid rows at the
// back cells and the new origin; launch_inflate_rects (mppi_costmap.h) derives again the float cells of the bands whose value the
// roll can change.  The kernels are k_costmap_roll.hip's; both tables live in the staging slot of the call (pinned, read in place).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mppi_costmap.h"
#include "mppi_kernels.h"

namespace ccv {

// One rolled map.  The exposed cells come from `strip` (null: every one of them is `fill`): first the row strip, the
// min(|dy|, ny) exposed rows over the full width in ascending new-frame iy, then the column strip, the min(|dx|, nx) exposed
// cells of each remaining row in ascending iy and ix.
struct alignas(16) RollEntry {
    const uint8_t* layer_src;   // [ny][nx] front
    uint8_t* layer_dst;         // [ny][nx] back
    const float* cells_src;     // [ny][nx] front: the grid rows that point here are the map's
    float* cells_dst;           // [ny][nx] back
    const uint8_t* strip;
    double origin_x, origin_y;  // of the rolled map, formed on the host
    int32_t nx, ny, dx, dy, fill, pad;
};
static_assert(sizeof(RollEntry) == 80, "a table of the staging slot");

// (the rectangles of k_inflate_rects are InflateArgs: the rectangle lies inside the map, layer and cells are the back ones)
constexpr int kRollMaxRects = 4;   // per map: a leading and a trailing band in x and in y

// Launch 1: n entries, the grid rows [B] of the handle.  (Launch 2: launch_inflate_rects.)
void launch_roll_shift(const RollEntry* entries, int32_t n, int64_t max_cells, GridRow* rows, int32_t B, hipStream_t stream);

}  // namespace ccv

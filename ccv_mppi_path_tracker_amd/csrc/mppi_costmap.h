// Costmaps inflated on the device (ccv_mppi_batch_set_occupancy / _update_occupancy_enqueue): the float
// cells the GRID kernels read (GridRow::cells, mppi_kernels.h) derived from a uint8 occupancy layer by an exact truncated
// Euclidean distance transform.  Integers and one table lookup:
//     occ(ix, iy)  = layer[iy * nx + ix] >= threshold             (a cell outside the map is not occupied)
//     D2(ix, iy)   = min over occupied (jx, jy) of (jx - ix)^2 + (jy - iy)^2
//     cost(ix, iy) = D2 <= R * R ? profile[D2] : free_value
// The kernels are k_costmap.hip's (the tile body: mppi_costmap_device.h); the host side (capi_batch_maps.hip) calls the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccv {

constexpr int kInflateMaxRadius = 64;   // CCV_MPPI_INFLATE_MAX_RADIUS
constexpr int kInflateTile = 64;        // a workgroup's output cells per axis
constexpr int kInflateSpan = kInflateTile + 2 * kInflateMaxRadius;   // ... and the cells it stages per axis at the largest R

// One inflation launch: the float cells of the rectangle (x0, y0, w, h) of one map, which lies inside the map, from the layer.
// Reads only `layer` and `profile`, writes only `cells`.
struct InflateArgs {
    const uint8_t* layer;   // [ny][nx]
    float* cells;           // [ny][nx]
    const float* profile;   // [R * R + 1]
    float free_value;
    int32_t nx, ny, threshold, R;
    int32_t x0, y0, w, h;
};
// the tiles of n cells of one axis, and of a w x h rectangle
constexpr int inflate_tiles(const int32_t n) { return (n + kInflateTile - 1) / kInflateTile; }
constexpr int inflate_tiles(const int32_t w, const int32_t h) { return inflate_tiles(w) * inflate_tiles(h); }
void launch_inflate(const InflateArgs& a, hipStream_t stream);
// The same over a table of n_rects rectangles of any maps in one launch (a roll's bands, a scan's boxes); max_tiles: inflate_tiles
// of the largest.  The table is read in place, from pinned host memory or device memory.  Defined in k_costmap_roll.hip.
void launch_inflate_rects(const InflateArgs* rects, int32_t n_rects, int32_t max_tiles, hipStream_t stream);

// The patch writer: the w x h rectangle at (x0, y0) of the layer [..][nx] from `patch` (row-major, tightly packed; pinned
// host memory or device memory).  The rectangle lies inside the map.
void launch_occupancy_patch(uint8_t* layer, int32_t nx, const uint8_t* patch, int32_t x0, int32_t y0, int32_t w, int32_t h, hipStream_t stream);

}  // namespace ccv

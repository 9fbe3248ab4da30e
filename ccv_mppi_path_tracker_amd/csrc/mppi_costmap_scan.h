// Laser scans traced into costmaps (ccv_mppi_batch_scan_occupancy_enqueue): every ray of a range scan
// clears the layer cells it passes through and, where it hit something, marks the cell it ends in.  Integers only.  With
// (sx, sy) the sensor's cell and (ex, ey) a ray's end cell, both in the map's current (rolled) frame:
//     adx = |ex - sx|, ady = |ey - sy|;  the major axis is x if adx >= ady, else y;  a = major length, b = minor length
//     cell i (0 <= i < a):  major = s_major + sign_major * i,  minor = s_minor + sign_minor * ((2 * i * b + a) div (2 * a))
// -- cell 0 is the sensor's, the end cell is not part of the ray, a ray with a = 0 has no cells.  a <= kScanMaxReach, so
// 2 * i * b + a < 2^26.  The layer after a call:
//     every ray cell inside the map = clear_value;  then, after ALL clears of that map, every end cell inside the map of a ray
//     with hit != 0 = mark_value
// and the float cells are the transform of mppi_costmap.h over the new layer: launch_inflate_rects (mppi_costmap.h) over one
// rectangle per entry.  The kernel is k_costmap_scan.hip's; the entry table and the rays live in the staging slot of the call
// (pinned host memory, read in place).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccv {

constexpr int kScanMaxReach = 4096;   // CCV_MPPI_SCAN_MAX_REACH
constexpr int kScanRayBytes = 9;      // of the staging slot per ray: the end cell (two int32) and the hit byte

// One scanned map: n_rays >= 1 rays from the cell (sx, sy), which lies inside the map.  All writes to one map come from the one
// workgroup of its entry.
struct alignas(16) ScanEntry {
    uint8_t* layer;          // [ny][nx] front
    const int32_t* end_xy;   // [n_rays][2]
    const uint8_t* hit;      // [n_rays]
    int32_t nx, ny, sx, sy, n_rays, clear_value, mark_value, pad;
};
static_assert(sizeof(ScanEntry) == 64, "a table of the staging slot");

// One launch for the n entries of a call.
void launch_scan_trace(const ScanEntry* entries, int32_t n, hipStream_t stream);

}  // namespace ccv

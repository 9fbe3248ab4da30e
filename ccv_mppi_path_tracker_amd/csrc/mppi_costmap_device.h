// Device side of the inflation (mppi_costmap.h): the body of one tile, written once for the two kernels
// that run it -- k_inflate (k_costmap.hip; one rectangle a launch, the grid its tiles) and k_inflate_rects (k_costmap_roll.hip;
// a table of rectangles a launch).  Each kernel keeps its own __shared__ arrays and hands them in.
#pragma once
#include "mppi_costmap.h"

namespace ccv {

constexpr int kInflateThreads = 256;   // of a workgroup of either kernel
constexpr int kNone = 255;   // row pass: no occupied cell within R in this row (R <= 64 < 255)

// One workgroup owns the tile (bx, by) of kInflateTile x kInflateTile output cells of the rectangle and stages the occupancy of
// the tile plus a halo of R cells (cells outside the map: free) into LDS, one byte per cell.  Row pass: for every staged row and
// every column of the tile, the distance g to the nearest occupied cell of that row within +-R (kNone: there is none).  Column
// pass: per output cell the minimum over |dy| <= R of g(x, y + dy)^2 + dy^2 in int32, then the table lookup and one float store.
// D2 <= R^2 implies |dx|, |dy| <= R, so the (2R + 1)^2 window decides it and the result is the exact truncated transform.  Both
// passes are O(R) per cell.  LDS (s_occ [kInflateSpan^2], s_g [kInflateSpan * kInflateTile]): 192 * 192 + 192 * 64 bytes = 48 KiB
// whatever R is, three workgroups to a CU's 160 KiB.
__device__ __forceinline__ void inflate_tile(const InflateArgs& a, const int bx, const int by, uint8_t* s_occ, uint8_t* s_g) {
    const int R = a.R, span = kInflateTile + 2 * R;
    const int tx0 = a.x0 + bx * kInflateTile, ty0 = a.y0 + by * kInflateTile;
    for (int i = threadIdx.x; i < span * span; i += kInflateThreads) {
        const int r = i / span, c = i - r * span;
        const int gx = tx0 - R + c, gy = ty0 - R + r;
        uint8_t o = 0;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny) o = (int)a.layer[(size_t)gy * a.nx + gx] >= a.threshold ? 1 : 0;
        s_occ[i] = o;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < span * kInflateTile; i += kInflateThreads) {
        const int r = i / kInflateTile, x = i - r * kInflateTile;
        const uint8_t* at = s_occ + r * span + x + R;   // (x + R - d >= 0 and x + R + d < span for d <= R)
        int g = kNone;
        for (int d = 0; d <= R; ++d)
            if (at[-d] | at[d]) {
                g = d;
                break;
            }
        s_g[i] = (uint8_t)g;
    }
    __syncthreads();
    const int x_end = a.x0 + a.w, y_end = a.y0 + a.h, R2 = R * R;
    for (int i = threadIdx.x; i < kInflateTile * kInflateTile; i += kInflateThreads) {
        const int y = i / kInflateTile, x = i - y * kInflateTile;
        const int gx = tx0 + x, gy = ty0 + y;
        if (gx >= x_end || gy >= y_end) continue;
        int best = R2 + 1;
        for (int dy = -R; dy <= R; ++dy) {
            const int g = s_g[(y + R + dy) * kInflateTile + x];
            const int d2 = g * g + dy * dy;   // (kNone^2 > R^2 + 1: never the minimum that counts)
            best = d2 < best ? d2 : best;
        }
        a.cells[(size_t)gy * a.nx + gx] = best <= R2 ? a.profile[best] : a.free_value;
    }
}

}  // namespace ccv

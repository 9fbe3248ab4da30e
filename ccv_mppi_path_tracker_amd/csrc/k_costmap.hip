// Costmap kernels (mppi_costmap.h): the patch writer and the inflation.  Neither is on the tick path of
// a handle without occupancy maps; no rollout, prologue or update kernel knows of them -- the GRID kernels read the float cells
// k_inflate leaves behind exactly as they read a caller's.
#include "mppi_costmap.h"

namespace ccv {
namespace {

constexpr int kThreads = 256;
constexpr int kNone = 255;   // row pass: no occupied cell within R in this row (R <= 64 < 255)

// Staging -> layer, one byte per cell.
__global__ __launch_bounds__(kThreads) void k_occupancy_patch(uint8_t* __restrict__ layer, const int nx, const uint8_t* __restrict__ patch,
                                                              const int x0, const int y0, const int w, const int h) {
    const int n = w * h;   // (<= CCV_MPPI_OCC_PATCH_MAX_CELLS = 2^20)
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const int r = i / w, c = i - r * w;
        layer[(size_t)(y0 + r) * nx + (x0 + c)] = patch[i];
    }
}

// One workgroup owns a tile of kInflateTile x kInflateTile output cells of the rectangle and stages the occupancy of the tile plus
// a halo of R cells (cells outside the map: free) into LDS, one byte per cell.  Row pass: for every staged row and every column of
// the tile, the distance g to the nearest occupied cell of that row within +-R (kNone: there is none).  Column pass: per output
// cell the minimum over |dy| <= R of g(x, y + dy)^2 + dy^2 in int32, then the table lookup and one float store.  D2 <= R^2
// implies |dx|, |dy| <= R, so the (2R + 1)^2 window decides it and the result is the exact truncated transform.  Both passes
// are O(R) per cell.  LDS: 192 * 192 + 192 * 64 bytes = 48 KiB whatever R is, three workgroups to a CU's 160 KiB.
__global__ __launch_bounds__(kThreads) void k_inflate(const InflateArgs a) {
    __shared__ uint8_t s_occ[kInflateSpan * kInflateSpan];
    __shared__ uint8_t s_g[kInflateSpan * kInflateTile];
    const int R = a.R, span = kInflateTile + 2 * R;
    const int tx0 = a.x0 + (int)blockIdx.x * kInflateTile, ty0 = a.y0 + (int)blockIdx.y * kInflateTile;
    for (int i = threadIdx.x; i < span * span; i += kThreads) {
        const int r = i / span, c = i - r * span;
        const int gx = tx0 - R + c, gy = ty0 - R + r;
        uint8_t o = 0;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny) o = (int)a.layer[(size_t)gy * a.nx + gx] >= a.threshold ? 1 : 0;
        s_occ[i] = o;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < span * kInflateTile; i += kThreads) {
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
    for (int i = threadIdx.x; i < kInflateTile * kInflateTile; i += kThreads) {
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

}  // namespace

void launch_inflate(const InflateArgs& a, hipStream_t stream) {
    const dim3 grid((a.w + kInflateTile - 1) / kInflateTile, (a.h + kInflateTile - 1) / kInflateTile);
    hipLaunchKernelGGL(k_inflate, grid, dim3(kThreads), 0, stream, a);
}

void launch_occupancy_patch(uint8_t* layer, const int32_t nx, const uint8_t* patch, const int32_t x0, const int32_t y0, const int32_t w,
                            const int32_t h, hipStream_t stream) {
    const int blocks = (w * h + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_occupancy_patch, dim3(blocks < 1024 ? blocks : 1024), dim3(kThreads), 0, stream, layer, nx, patch, x0, y0, w, h);
}

}  // namespace ccv

// Costmap kernels (mppi_costmap.h): the patch writer and the inflation.  Neither is on the tick path of
// a handle without occupancy maps; no rollout, prologue or update kernel knows of them -- the GRID kernels read the float cells
// k_inflate leaves behind exactly as they read a caller's.
#include "mppi_costmap_device.h"

namespace ccv {
namespace {

constexpr int kThreads = kInflateThreads;

// Staging -> layer, one byte per cell.
__global__ __launch_bounds__(kThreads) void k_occupancy_patch(uint8_t* __restrict__ layer, const int nx, const uint8_t* __restrict__ patch,
                                                              const int x0, const int y0, const int w, const int h) {
    const int n = w * h;   // (<= CCV_MPPI_OCC_PATCH_MAX_CELLS = 2^20)
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const int r = i / w, c = i - r * w;
        layer[(size_t)(y0 + r) * nx + (x0 + c)] = patch[i];
    }
}

// blockIdx.x, blockIdx.y: the tile of the rectangle (inflate_tile, mppi_costmap_device.h).
__global__ __launch_bounds__(kThreads) void k_inflate(const InflateArgs a) {
    __shared__ uint8_t s_occ[kInflateSpan * kInflateSpan];
    __shared__ uint8_t s_g[kInflateSpan * kInflateTile];
    inflate_tile(a, (int)blockIdx.x, (int)blockIdx.y, s_occ, s_g);
}

}  // namespace

void launch_inflate(const InflateArgs& a, hipStream_t stream) {
    const dim3 grid(inflate_tiles(a.w), inflate_tiles(a.h));
    hipLaunchKernelGGL(k_inflate, grid, dim3(kThreads), 0, stream, a);
}

void launch_occupancy_patch(uint8_t* layer, const int32_t nx, const uint8_t* patch, const int32_t x0, const int32_t y0, const int32_t w,
                            const int32_t h, hipStream_t stream) {
    const int blocks = (w * h + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_occupancy_patch, dim3(blocks < 1024 ? blocks : 1024), dim3(kThreads), 0, stream, layer, nx, patch, x0, y0, w, h);
}

}  // namespace ccv

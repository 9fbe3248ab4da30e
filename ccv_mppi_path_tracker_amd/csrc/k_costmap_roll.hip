// Rolling-costmap kernels (mppi_costmap_roll.h): the shift and the inflation of the bands.  Neither is
// on the tick path of a handle that never rolls; no rollout, prologue or update kernel knows of them -- the GRID kernels read
// the grid rows afresh at every launch and find the back cells and the new origin there.
#include "mppi_costmap_roll.h"
#include "mppi_costmap_device.h"

namespace ccv {
namespace {

constexpr int kThreads = kInflateThreads;

// blockIdx.y: the entry.  Out of place: the back layer and the back float cells from the front ones at the shifted index (a
// float cell whose source lies outside the map is in a band and is k_inflate_rects' to write), the exposed layer cells from the
// strips or `fill`.  The first workgroup of an entry also moves the grid rows of the instances on the map (row.cells == the
// front cells) to the back cells and the new origin: later launches read the rows in stream order.
__global__ __launch_bounds__(kThreads) void k_roll_shift(const RollEntry* __restrict__ entries, GridRow* __restrict__ rows, const int B) {
    const RollEntry e = entries[blockIdx.y];
    const int nx = e.nx, ny = e.ny, dx = e.dx, dy = e.dy;
    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const int ax = adx < nx ? adx : nx, ay = ady < ny ? ady : ny;   // exposed columns of a row, exposed rows
    const int row0 = dy > 0 ? ny - ay : 0, col0 = dx > 0 ? nx - ax : 0;   // where they start in the new frame
    const int n = nx * ny;   // (<= CCV_MPPI_GRID_MAX_CELLS = 2^26)
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const int iy = i / nx, ix = i - iy * nx;
        const int64_t sx = (int64_t)ix + dx, sy = (int64_t)iy + dy;
        if (sx >= 0 && sx < nx && sy >= 0 && sy < ny) {
            const size_t s = (size_t)sy * nx + (size_t)sx;
            e.layer_dst[i] = e.layer_src[s];
            e.cells_dst[i] = e.cells_src[s];
            continue;
        }
        int v = e.fill;
        if (e.strip) {
            if (iy >= row0 && iy < row0 + ay) v = e.strip[(size_t)(iy - row0) * nx + ix];
            else v = e.strip[(size_t)ay * nx + (size_t)(dy < 0 ? iy - ay : iy) * ax + (ix - col0)];
        }
        e.layer_dst[i] = (uint8_t)v;
    }
    if (blockIdx.x != 0) return;
    for (int b = threadIdx.x; b < B; b += kThreads)
        if (rows[b].cells == e.cells_src) {
            rows[b].origin_x = e.origin_x;
            rows[b].origin_y = e.origin_y;
            rows[b].cells = e.cells_dst;
        }
}

// blockIdx.y: the rectangle, blockIdx.x: its tile, row-major; the tiles past a rectangle's end exit.  The body is k_inflate's
// (inflate_tile, mppi_costmap_device.h).
__global__ __launch_bounds__(kThreads) void k_inflate_rects(const InflateArgs* __restrict__ rects) {
    __shared__ uint8_t s_occ[kInflateSpan * kInflateSpan];
    __shared__ uint8_t s_g[kInflateSpan * kInflateTile];
    const InflateArgs a = rects[blockIdx.y];
    const int tiles_x = inflate_tiles(a.w);
    if ((int)blockIdx.x >= inflate_tiles(a.w, a.h)) return;
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    inflate_tile(a, bx, by, s_occ, s_g);
}

}  // namespace

void launch_roll_shift(const RollEntry* entries, const int32_t n, const int64_t max_cells, GridRow* rows, const int32_t B, hipStream_t stream) {
    // (eight cells to a thread: every workgroup starts by reading its entry out of the staging slot, which is host memory)
    const int64_t blocks = (max_cells + 8 * kThreads - 1) / (8 * kThreads);
    hipLaunchKernelGGL(k_roll_shift, dim3((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)n), dim3(kThreads), 0, stream, entries, rows, B);
}

// (declared in mppi_costmap.h beside launch_inflate: the roll and the scan both launch it)
void launch_inflate_rects(const InflateArgs* rects, const int32_t n_rects, const int32_t max_tiles, hipStream_t stream) {
    hipLaunchKernelGGL(k_inflate_rects, dim3((unsigned)max_tiles, (unsigned)n_rects), dim3(kThreads), 0, stream, rects);
}

}  // namespace ccv

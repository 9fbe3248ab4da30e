// Costmaps that follow their robots (mppi_costmap_follow.h): the decision and the shift.  Not on the tick
// path of a handle that never follows; no rollout, prologue or update kernel knows of it -- the GRID kernels read the grid rows
// afresh at every launch and find the back cells and the new origin there.  The bands' float cells follow in the next launch
// (k_inflate_rects, k_costmap_roll.hip) over the rectangles this kernel writes.
#include "mppi_costmap_follow.h"
#include "mppi_costmap_rects.h"

namespace ccv {
namespace {

constexpr int kThreads = 256;
static_assert(kFollowRects == kRollBands, "a follow's rectangles are a roll's bands");

// blockIdx.y: the entry.  Every workgroup forms the decision from the same two reads (the pose and the map's current frame
// slot: nothing in this launch writes either) and so arrives at the same (dx, dy): no flag, no atomic, no wait.  Then
// k_roll_shift's loop (k_costmap_roll.hip) with every exposed cell `fill`; where nothing moves it is a copy, the same for all
// workgroups.  The first workgroup of an entry writes the other frame slot, the result row, the four rectangles and the grid rows
// of the instances on the map.
__global__ __launch_bounds__(kThreads) void k_follow_shift(const FollowEntry* __restrict__ entries, InflateArgs* __restrict__ rects,
                                                           GridRow* __restrict__ rows, const int B) {
    const FollowEntry e = entries[blockIdx.y];
    const FollowFrame f = *e.frame_src;
    const FollowDecision d = follow_decide(e.pose[0], e.pose[1], f, e.ox0, e.oy0, e.resolution, e.inv, e.nx, e.ny, e.margin, e.max_step);
    const int nx = e.nx, ny = e.ny, dx = d.dx, dy = d.dy;   // (|dx|, |dy| <= max_step <= CCV_MPPI_GRID_MAX_DIM)
    const int n = nx * ny;   // (<= CCV_MPPI_GRID_MAX_CELLS = 2^26)
    const uint8_t fill = (uint8_t)e.fill;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const int iy = i / nx, ix = i - iy * nx;
        const int sx = ix + dx, sy = iy + dy;
        if (sx >= 0 && sx < nx && sy >= 0 && sy < ny) {
            const size_t s = (size_t)sy * nx + (size_t)sx;
            e.layer_dst[i] = e.layer_src[s];
            e.cells_dst[i] = e.cells_src[s];
        } else {
            e.layer_dst[i] = fill;   // (its float cell lies in a band)
        }
    }
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        *e.frame_dst = d.frame;
        e.result[0] = d.status;
        e.result[1] = dx;
        e.result[2] = dy;
        e.result[3] = 0;
        Rect band[kRollBands];
        const int n_bands = d.status == kFollowMoved ? roll_bands(nx, ny, dx, dy, e.rect.R, band) : 0;
        for (int k = 0; k < kRollBands; ++k) {
            InflateArgs r = e.rect;
            r.x0 = r.y0 = r.w = r.h = 0;
            if (k < n_bands) {
                r.x0 = band[k].x0;
                r.y0 = band[k].y0;
                r.w = band[k].w;
                r.h = band[k].h;
            }
            rects[(size_t)blockIdx.y * kRollBands + k] = r;
        }
    }
    for (int b = threadIdx.x; b < B; b += kThreads)
        if (rows[b].cells == e.cells_src) {
            rows[b].origin_x = d.frame.origin_x;
            rows[b].origin_y = d.frame.origin_y;
            rows[b].cells = e.cells_dst;
        }
}

// a thread per entry: the sensing entries of a call, completed from the maps' current frame slots
__global__ __launch_bounds__(kThreads) void k_follow_resolve_sense(const SenseFollowEntry* __restrict__ in, SenseEntry* __restrict__ out, const int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    SenseEntry e = in[i].entry;
    const FollowFrame f = *in[i].frame;
    e.off_x = (int32_t)(e.off_x + f.cx);
    e.off_y = (int32_t)(e.off_y + f.cy);
    out[i] = e;
}

__device__ __forceinline__ int goal_cell(const double p, const double origin, const double inv, const int n) {
    const double f = (p - origin) * inv;
    return !(f >= 0.0) ? 0 : f >= (double)n ? n - 1 : (int)f;
}

// ... and the planning entries
__global__ __launch_bounds__(kThreads) void k_follow_resolve_plan(const PlanFollowEntry* __restrict__ in, PlanEntry* __restrict__ out, const int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const PlanFollowEntry w = in[i];
    PlanEntry e = w.entry;
    const FollowFrame f = *w.frame;
    e.origin_x = f.origin_x;
    e.origin_y = f.origin_y;
    if (w.world_goal) {
        e.goal_x = goal_cell(w.goal_wx, e.origin_x, e.inv, e.nx);
        e.goal_y = goal_cell(w.goal_wy, e.origin_y, e.inv, e.ny);
    }
    out[i] = e;
}

}  // namespace

void launch_follow_resolve_sense(const SenseFollowEntry* in, SenseEntry* out, const int32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_follow_resolve_sense, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, in, out, n);
}

void launch_follow_resolve_plan(const PlanFollowEntry* in, PlanEntry* out, const int32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_follow_resolve_plan, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, in, out, n);
}

void launch_follow_shift(const FollowEntry* entries, InflateArgs* rects, const int32_t n, const int64_t max_cells, GridRow* rows, const int32_t B,
                         hipStream_t stream) {
    // (eight cells to a thread, as launch_roll_shift: every workgroup starts by reading its entry out of the staging slot)
    const int64_t blocks = (max_cells + 8 * kThreads - 1) / (8 * kThreads);
    hipLaunchKernelGGL(k_follow_shift, dim3((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)n), dim3(kThreads), 0, stream, entries, rects, rows, B);
}

}  // namespace ccv

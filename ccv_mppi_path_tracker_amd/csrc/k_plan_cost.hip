// Paths planned on the device with traversal weights from the cell costs (mppi_plan_cost.h): k_plan.hip's
// kernel -- one workgroup per entry, the field in LDS, strips relaxed forward and backward, two stamped flags, a single-lane
// descent -- with every step out of a cell multiplied by that cell's m = 1 + q.  A unit of its own with a body of its own:
// k_plan.hip is what it was, instruction for instruction, and is what runs while every multiplier is 1.  The multipliers do not
// fit beside the largest field in LDS, so a relaxation forms its cell's from the float map in global memory (L2-resident: at
// most 320 KB), loaded kAhead cells ahead of the relaxation that uses it: the load does not wait for the LDS reads before it.
#include "mppi_plan_cost.h"

namespace ccv {
namespace {

constexpr int kThreads = 1024;
constexpr int kAhead = 4;   // cells a strip's loads run ahead of its relaxations
// the field's image, pitch and flags: k_plan.hip's, cell for cell
constexpr int kFieldCells = kPlanMaxField - 2;

__device__ __forceinline__ int plan_cost_pitch(const int nx, const int ny) {
    const int p0 = nx + 1, p1 = p0 + ((6 - (p0 & 3)) & 3);
    return (ny + 2) * p1 + 1 <= kFieldCells ? p1 : p0;
}

__device__ __forceinline__ bool plan_cost_blocked(const float v, const float lethal) { return !(v <= lethal); }

// D(c) = min(D(c), min(kPlanFar, D(n) + w * m(c))) over the eight neighbours of the free cell c, whose float value is v; whether
// D(c) fell.  Values another thread is lowering meanwhile are read old or new: both are bounds from above that the fixpoint
// lies under.  A blocked cell and the goal return before the multiplier is formed.
__device__ __forceinline__ bool plan_cost_relax(uint16_t* const f, const int c, const int P, const float v, const float gain, const int32_t max_penalty) {
    const uint32_t d = f[c];
    if (d == kPlanBlocked || d == 0u) return false;
    const uint32_t m = plan_multiplier(v, gain, max_penalty);
    const uint32_t e = f[c + 1], w = f[c - 1], n = f[c + P], s = f[c - P];
    const uint32_t ne = f[c + P + 1], nw = f[c + P - 1], sw = f[c - P - 1], se = f[c - P + 1];
    const bool fe = e != kPlanBlocked, fw = w != kPlanBlocked, fn = n != kPlanBlocked, fs = s != kPlanBlocked;
    // (a blocked neighbour, 65535, gives at least 65540: never below d, which is at most kPlanFar; 65535 + 7 * 16 fits 32 bits)
    uint32_t best = min(min(e, w), min(n, s)) + 5u * m;
    uint32_t diag = kPlanBlocked;
    if (fe && fn) diag = min(diag, ne);
    if (fw && fn) diag = min(diag, nw);
    if (fw && fs) diag = min(diag, sw);
    if (fe && fs) diag = min(diag, se);
    best = min(best, diag + 7u * m);
    best = min(best, kPlanFar);
    if (best >= d) return false;
    f[c] = (uint16_t)best;
    return true;
}

// blockIdx.x: the entry.  k_plan_field's sweep: every row and every column is a strip owned by one thread.  The strip's floats:
// a row owner walks consecutive floats of its row, the column owners of a wave read neighbouring floats of one row at a time.
// Every index into the map stays inside the strip: a load ahead is clamped to the strip's last (going back: first) cell.
__global__ __launch_bounds__(kThreads) void k_plan_field_cost(const PlanEntry* __restrict__ entries, const float lethal, const int max_sweeps,
                                                               const float gain, const int32_t max_penalty) {
    __shared__ uint16_t s_field[kFieldCells + 2];
    uint16_t* const s_flag = s_field + kFieldCells;
    const PlanEntry e = entries[blockIdx.x];
    const int nx = e.nx, ny = e.ny;
    const double fx = (e.pose[0] - e.origin_x) * e.inv, fy = (e.pose[1] - e.origin_y) * e.inv;
    const bool in = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny;
    const int sx = in ? (int)fx : -1, sy = in ? (int)fy : -1;
    int32_t early = 0;
    if (!in) early = kPlanNoStart;
    else if (plan_cost_blocked(e.cells[(size_t)sy * nx + sx], lethal)) early = kPlanStartBlocked;
    else if (plan_cost_blocked(e.cells[(size_t)e.goal_y * nx + e.goal_x], lethal)) early = kPlanGoalBlocked;
    if (early) {   // (the whole workgroup, from the same three loads: no barrier is passed)
        if (threadIdx.x == 0) {
            e.result[0] = early;
            e.result[1] = 0;
            e.result[2] = sx;
            e.result[3] = sy;
            e.result[4] = -1;
            e.result[5] = 0;
        }
        return;
    }
    const int P = plan_cost_pitch(nx, ny), total = (ny + 2) * P + 1;
    for (int i = threadIdx.x; i < total; i += kThreads) {
        const int y = i / P - 1, x = i % P - 1;
        uint32_t d = kPlanBlocked;
        if (x >= 0 && x < nx && y >= 0 && y < ny && !plan_cost_blocked(e.cells[(size_t)y * nx + x], lethal)) d = x == e.goal_x && y == e.goal_y ? 0u : kPlanFar;
        s_field[i] = (uint16_t)d;
    }
    if (threadIdx.x < 2) s_flag[threadIdx.x] = 0;
    __syncthreads();
    int sweeps = 0;
    bool converged = false;
    while (sweeps < max_sweeps) {
        ++sweeps;
        int changed = 0;
        for (int item = threadIdx.x; item < ny + nx; item += kThreads) {
            const bool row = item < ny;
            const int base = row ? (item + 1) * P + 1 : P + (item - ny) + 1, step = row ? 1 : P, len = row ? nx : ny;
            const float* const g = e.cells + (row ? (size_t)item * nx : (size_t)(item - ny));
            const size_t gstep = row ? (size_t)1 : (size_t)nx;
            // kAhead cells' floats are in registers while the kAhead before them are relaxed
            float v[kAhead], ahead[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) v[k] = g[(size_t)min(k, len - 1) * gstep];
            for (int i0 = 0; i0 < len; i0 += kAhead) {
#pragma unroll
                for (int k = 0; k < kAhead; ++k) ahead[k] = g[(size_t)min(i0 + kAhead + k, len - 1) * gstep];
#pragma unroll
                for (int k = 0; k < kAhead; ++k)
                    if (i0 + k < len) changed |= (int)plan_cost_relax(s_field, base + (i0 + k) * step, P, v[k], gain, max_penalty);
#pragma unroll
                for (int k = 0; k < kAhead; ++k) v[k] = ahead[k];
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k) v[k] = g[(size_t)max(len - 2 - k, 0) * gstep];
            for (int i0 = len - 2; i0 >= 0; i0 -= kAhead) {
#pragma unroll
                for (int k = 0; k < kAhead; ++k) ahead[k] = g[(size_t)max(i0 - kAhead - k, 0) * gstep];
#pragma unroll
                for (int k = 0; k < kAhead; ++k)
                    if (i0 - k >= 0) changed |= (int)plan_cost_relax(s_field, base + (i0 - k) * step, P, v[k], gain, max_penalty);
#pragma unroll
                for (int k = 0; k < kAhead; ++k) v[k] = ahead[k];
            }
        }
        if (changed) s_flag[sweeps & 1] = (uint16_t)sweeps;
        __syncthreads();
        if (s_flag[sweeps & 1] != (uint16_t)sweeps) {
            converged = true;
            break;
        }
    }
    if (threadIdx.x == 0) {
        const int at = (sy + 1) * P + sx + 1;
        const uint32_t ds = s_field[at];
        int32_t status = kPlanOk, L = 0;
        if (!converged) status = kPlanNotConverged;
        else if (ds == kPlanFar) status = kPlanUnreachable;
        else {
            // the descent: D falls by at least 5 a step, so at most 65532 / 5 + 1 cells are visited
            int c = at;
            uint32_t d = ds;
            for (;;) {
                const int x = c % P - 1, y = c / P - 1;
                if (L < e.capacity) {
                    e.path_x[L] = e.origin_x + ((double)x + 0.5) * e.resolution;
                    e.path_y[L] = e.origin_y + ((double)y + 0.5) * e.resolution;
                }
                ++L;
                if (d == 0u || L >= kPlanMaxPoses) break;
                // the cell the descent stands on is the cell that is left: its multiplier, read once
                const uint32_t m = plan_multiplier(e.cells[(size_t)y * nx + x], gain, max_penalty);
                const uint32_t ws = 5u * m, wd = 7u * m;
                const uint32_t ce = s_field[c + 1], cn = s_field[c + P], cw = s_field[c - 1], cs = s_field[c - P];
                const bool fe = ce != kPlanBlocked, fn = cn != kPlanBlocked, fw = cw != kPlanBlocked, fs = cs != kPlanBlocked;
                int next = c;
                if (ce + ws == d) next = c + 1;
                else if (cn + ws == d) next = c + P;
                else if (cw + ws == d) next = c - 1;
                else if (cs + ws == d) next = c - P;
                else if (fe && fn && s_field[c + P + 1] + wd == d) next = c + P + 1;
                else if (fw && fn && s_field[c + P - 1] + wd == d) next = c + P - 1;
                else if (fw && fs && s_field[c - P - 1] + wd == d) next = c - P - 1;
                else if (fe && fs && s_field[c - P + 1] + wd == d) next = c - P + 1;
                if (next == c) break;   // (not at a fixpoint: cannot happen after a sweep without a change)
                c = next;
                d = s_field[c];
            }
            if (L > e.capacity) status = kPlanTruncated;
            e.inst->n_path = L < e.capacity ? L : e.capacity;
        }
        e.result[0] = status;
        e.result[1] = L;
        e.result[2] = sx;
        e.result[3] = sy;
        e.result[4] = converged ? (int32_t)ds : -1;
        e.result[5] = sweeps;
    }
    if (e.field && converged)
        for (int i = threadIdx.x; i < nx * ny; i += kThreads) e.field[i] = s_field[(i / nx + 1) * P + i % nx + 1];
}

}  // namespace

void launch_plan_field_cost(const PlanEntry* entries, const int32_t n, const float lethal, const int32_t max_sweeps, const float gain,
                            const int32_t max_penalty, hipStream_t stream) {
    hipLaunchKernelGGL(k_plan_field_cost, dim3((unsigned)n), dim3(kThreads), 0, stream, entries, lethal, max_sweeps, gain, max_penalty);
}

}  // namespace ccv

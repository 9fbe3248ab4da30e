// Paths planned on the device (mppi_plan.h): the distance field of every named instance's map relaxed to
// its fixpoint in LDS, the descent from the cell the resident pose lies in, and the instance's path slice and n_path written in
// stream order.  Not on the tick path of a handle that never plans; no rollout, prologue or update kernel knows of it -- the
// next tick's prologue reads BatchInstance::n_path and the path from device memory as it always does.
#include "mppi_plan.h"

namespace ccv {
namespace {

constexpr int kThreads = 1024;
// The field in LDS, uint16, with a border of blocked cells: cell (x, y), -1 <= x <= nx, -1 <= y <= ny, at (y + 1) * P + (x + 1).
// P >= nx + 1: the right border of row y IS the left border of row y + 1, so the image has (ny + 2) * P + 1 cells, at most
// (nx + 2)(ny + 2) - (ny + 1) <= kPlanMaxField - 2 -- the two cells that leaves of the CU's 160 KiB are the sweeps' "a cell
// fell" flags.  (__syncthreads_or would be the one-line way to that answer, but its reduction takes 260 bytes of LDS of its own
// and LDS atomics: beside the largest field the kernel then does not link.)
constexpr int kFieldCells = kPlanMaxField - 2;

// the pitch: nx + 1 rounded up to 2 mod 4 where the image still fits -- the lanes of a wave that walk neighbouring rows then
// hit 32 different banks (bank = (byte address / 4) mod 32; a pitch of 0 mod 64 would put all of them on one)
__device__ __forceinline__ int plan_pitch(const int nx, const int ny) {
    const int p0 = nx + 1, p1 = p0 + ((6 - (p0 & 3)) & 3);
    return (ny + 2) * p1 + 1 <= kFieldCells ? p1 : p0;
}

__device__ __forceinline__ bool plan_blocked(const float v, const float lethal) { return !(v <= lethal); }

// D(c) = min(D(c), min(kPlanFar, D(n) + w)) over the eight neighbours of the free cell c; whether D(c) fell.  Values another
// thread is lowering meanwhile are read old or new: both are bounds from above that the fixpoint lies under.
__device__ __forceinline__ bool plan_relax(uint16_t* const f, const int c, const int P) {
    const uint32_t d = f[c];
    if (d == kPlanBlocked || d == 0u) return false;
    const uint32_t e = f[c + 1], w = f[c - 1], n = f[c + P], s = f[c - P];
    const uint32_t ne = f[c + P + 1], nw = f[c + P - 1], sw = f[c - P - 1], se = f[c - P + 1];
    const bool fe = e != kPlanBlocked, fw = w != kPlanBlocked, fn = n != kPlanBlocked, fs = s != kPlanBlocked;
    // (a blocked neighbour, 65535, gives 65540 or 65542: never below d, which is at most kPlanFar)
    uint32_t best = min(min(e, w), min(n, s)) + 5u;
    uint32_t diag = kPlanBlocked;
    if (fe && fn) diag = min(diag, ne);
    if (fw && fn) diag = min(diag, nw);
    if (fw && fs) diag = min(diag, sw);
    if (fe && fs) diag = min(diag, se);
    best = min(best, diag + 7u);
    best = min(best, kPlanFar);
    if (best >= d) return false;
    f[c] = (uint16_t)best;
    return true;
}

// blockIdx.x: the entry; one workgroup per entry.  A sweep: every row and every column of the map is a strip owned by one
// thread, which relaxes its cells serially forward and then backward -- the front crosses a strip's free run in one sweep
// instead of moving one cell, and a corridor map converges in about as many sweeps as it has corridors.  Rows and columns run
// side by side in one phase; one barrier per sweep.  Whether any cell fell: sweep k's threads that lowered a cell store the
// stamp (uint16_t)k to flag k & 1 -- the same value from all of them, a plain store -- and after the barrier every thread reads
// it.  The flag still holds sweep k - 2's stamp otherwise (that sweep changed something, or the loop had ended), which differs
// from k's; sweep k + 1 writes the other flag, and sweep k + 2's writers have passed barrier k + 1, so no reader is overtaken.
__global__ __launch_bounds__(kThreads) void k_plan_field(const PlanEntry* __restrict__ entries, const float lethal, const int max_sweeps) {
    __shared__ uint16_t s_field[kFieldCells + 2];
    uint16_t* const s_flag = s_field + kFieldCells;
    const PlanEntry e = entries[blockIdx.x];
    const int nx = e.nx, ny = e.ny;
    // the start cell: one subtraction, one multiplication (the unit is built without contraction), fp64 compares
    const double fx = (e.pose[0] - e.origin_x) * e.inv, fy = (e.pose[1] - e.origin_y) * e.inv;
    const bool in = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny;
    const int sx = in ? (int)fx : -1, sy = in ? (int)fy : -1;
    int32_t early = 0;
    if (!in) early = kPlanNoStart;
    else if (plan_blocked(e.cells[(size_t)sy * nx + sx], lethal)) early = kPlanStartBlocked;
    else if (plan_blocked(e.cells[(size_t)e.goal_y * nx + e.goal_x], lethal)) early = kPlanGoalBlocked;
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
    const int P = plan_pitch(nx, ny), total = (ny + 2) * P + 1;
    for (int i = threadIdx.x; i < total; i += kThreads) {
        const int y = i / P - 1, x = i % P - 1;
        uint32_t d = kPlanBlocked;
        if (x >= 0 && x < nx && y >= 0 && y < ny && !plan_blocked(e.cells[(size_t)y * nx + x], lethal)) d = x == e.goal_x && y == e.goal_y ? 0u : kPlanFar;
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
            for (int i = 0; i < len; ++i) changed |= (int)plan_relax(s_field, base + i * step, P);
            for (int i = len - 2; i >= 0; --i) changed |= (int)plan_relax(s_field, base + i * step, P);
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
                if (L < e.capacity) {
                    const int x = c % P - 1, y = c / P - 1;
                    e.path_x[L] = e.origin_x + ((double)x + 0.5) * e.resolution;
                    e.path_y[L] = e.origin_y + ((double)y + 0.5) * e.resolution;
                }
                ++L;
                if (d == 0u || L >= kPlanMaxPoses) break;
                const uint32_t ce = s_field[c + 1], cn = s_field[c + P], cw = s_field[c - 1], cs = s_field[c - P];
                const bool fe = ce != kPlanBlocked, fn = cn != kPlanBlocked, fw = cw != kPlanBlocked, fs = cs != kPlanBlocked;
                int next = c;
                if (ce + 5u == d) next = c + 1;
                else if (cn + 5u == d) next = c + P;
                else if (cw + 5u == d) next = c - 1;
                else if (cs + 5u == d) next = c - P;
                else if (fe && fn && s_field[c + P + 1] + 7u == d) next = c + P + 1;
                else if (fw && fn && s_field[c + P - 1] + 7u == d) next = c + P - 1;
                else if (fw && fs && s_field[c - P - 1] + 7u == d) next = c - P - 1;
                else if (fe && fs && s_field[c - P + 1] + 7u == d) next = c - P + 1;
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

void launch_plan_field(const PlanEntry* entries, const int32_t n, const float lethal, const int32_t max_sweeps, hipStream_t stream) {
    hipLaunchKernelGGL(k_plan_field, dim3((unsigned)n), dim3(kThreads), 0, stream, entries, lethal, max_sweeps);
}

}  // namespace ccv

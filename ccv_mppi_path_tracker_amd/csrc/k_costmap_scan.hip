// Scan tracing (mppi_costmap_scan.h): the rays of a call's range scans written into the occupancy layers.
// Not on the tick path of a handle that is given no scans; no rollout, prologue or update kernel knows of it -- the float cells
// follow in the next launch (k_inflate_rects, k_costmap_roll.hip), and the GRID kernels read those.
#include "mppi_costmap_scan.h"

namespace ccv {
namespace {

constexpr int kThreads = 1024;
constexpr int kWave = 64;

// blockIdx.x: the entry; one workgroup per entry, so that every write to a map comes from one workgroup and the one ordering
// the call promises -- marks after all clears -- is a workgroup barrier.  Clear phase: a wave per ray, its lanes striding over
// the ray's cells (closed form: any lane computes any cell), so that an x-major ray stores adjacent bytes.  Mark phase: a thread
// per ray.  Every clear stores the same byte and every mark the same byte, so the layer does not depend on the workgroup's
// width or on how rays are dealt to waves.  Byte stores only.
__global__ __launch_bounds__(kThreads) void k_scan_trace(const ScanEntry* __restrict__ entries) {
    const ScanEntry e = entries[blockIdx.x];
    const int nx = e.nx, ny = e.ny, sx = e.sx, sy = e.sy, n = e.n_rays;
    const uint8_t clear = (uint8_t)e.clear_value, mark = (uint8_t)e.mark_value;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, waves = blockDim.x / kWave;
    // A round is waves * 64 rays, ray base + j * waves + wave the j-th of this wave: lane j fetches it (the slot is host memory:
    // one trip for the wave's 64 rays, not one per ray) and hands it to all lanes when its turn comes.
    for (int base = 0; base < n; base += waves * kWave) {
        const int mine = base + lane * waves + wave;
        int mdx = 0, mdy = 0;
        if (mine < n) {
            mdx = e.end_xy[2 * (size_t)mine] - sx;   // (|dx|, |dy| <= kScanMaxReach: the host's check)
            mdy = e.end_xy[2 * (size_t)mine + 1] - sy;
        }
        const int left = (n - base - wave + waves - 1) / waves, count = left < kWave ? left : kWave;   // this wave's rays of the round
        for (int j = 0; j < count; ++j) {
            const int dx = __shfl(mdx, j), dy = __shfl(mdy, j);
            const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
            const int stepx = dx < 0 ? -1 : 1, stepy = dy < 0 ? -1 : 1;
            const bool xmajor = adx >= ady;
            const unsigned a = (unsigned)(xmajor ? adx : ady), b = (unsigned)(xmajor ? ady : adx);
            for (unsigned i = (unsigned)lane; i < a; i += kWave) {
                const int minor = (int)((2u * i * b + a) / (2u * a));   // (< 2^26)
                const int x = sx + stepx * (xmajor ? (int)i : minor), y = sy + stepy * (xmajor ? minor : (int)i);
                if (x >= 0 && x < nx && y >= 0 && y < ny) e.layer[(size_t)y * nx + x] = clear;
            }
        }
    }
    // every wave's clears have left it, and are visible at workgroup scope, before any wave marks
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        if (!e.hit[r]) continue;
        const int x = e.end_xy[2 * (size_t)r], y = e.end_xy[2 * (size_t)r + 1];
        if (x >= 0 && x < nx && y >= 0 && y < ny) e.layer[(size_t)y * nx + x] = mark;
    }
}

}  // namespace

void launch_scan_trace(const ScanEntry* entries, const int32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_scan_trace, dim3((unsigned)n), dim3(kThreads), 0, stream, entries);
}

}  // namespace ccv

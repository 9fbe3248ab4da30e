// The simulated range sensor (mppi_costmap_sense.h): every named robot's beams cast through the world map
// from its resident pose, the result written into its occupancy layer.  Not on the tick path of a handle that never senses; no
// rollout, prologue or update kernel knows of it -- the float cells follow in the next launch (k_inflate_rects,
// k_costmap_roll.hip) over the rectangles this kernel writes, and the GRID kernels read those.
#include "mppi_costmap_sense.h"

namespace ccv {
namespace {

constexpr int kThreads = 1024;
constexpr int kWave = 64;

// cell i of the beam (dx, dy) from (sx, sy): mppi_costmap_scan.h's closed form (a >= 1, i <= a <= kScanMaxReach: below 2^26)
struct Beam {
    int stepx, stepy;
    bool xmajor;
    unsigned a, b;
    __device__ __forceinline__ Beam(const int dx, const int dy) {
        const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        stepx = dx < 0 ? -1 : 1;
        stepy = dy < 0 ? -1 : 1;
        xmajor = adx >= ady;
        a = (unsigned)(xmajor ? adx : ady);
        b = (unsigned)(xmajor ? ady : adx);
    }
    __device__ __forceinline__ void cell(const int sx, const int sy, const unsigned i, int& x, int& y) const {
        const int minor = (int)((2u * i * b + a) / (2u * a));
        x = sx + stepx * (xmajor ? (int)i : minor);
        y = sy + stepy * (xmajor ? minor : (int)i);
    }
};

// blockIdx.x: the entry; one workgroup per entry, so that every write to a map comes from one workgroup and "marks after all
// clears" is a workgroup barrier (k_scan_trace's shape).  Search and clear: a wave per beam, its lanes striding over the beam's
// cells in chunks of 64 -- a lane loads one world byte, the ballot's first set bit is the blocked cell, the chunk loop ends at
// the first blocked chunk, and the same lanes store the clear byte to the local cells below it.  Mark: a thread per beam, from
// the blocked cells the waves left in LDS.  Every clear stores the same byte and every mark the same byte, so the layer does not
// depend on how beams are dealt to waves.  Byte and dword stores only.
__global__ __launch_bounds__(kThreads) void k_sense_trace(const SenseEntry* __restrict__ entries, InflateArgs* __restrict__ rects, const SenseArgs A) {
    __shared__ int32_t s_first[kSenseMaxBeams];
    const SenseEntry e = entries[blockIdx.x];
    const int nx = e.rect.nx, ny = e.rect.ny, n = A.n_beams;
    // the robot's world cell: one subtraction, one multiplication (the unit is built without contraction), fp64 compares
    const double fx = (e.pose[0] - A.origin_x) * A.inv, fy = (e.pose[1] - A.origin_y) * A.inv;
    const bool in = fx >= 0.0 && fx < (double)A.wnx && fy >= 0.0 && fy < (double)A.wny;
    const int sx = in ? (int)fx : -1, sy = in ? (int)fy : -1;
    const int lx = sx - e.off_x, ly = sy - e.off_y;   // (|off| <= 2^30, s < 2^15)
    if (threadIdx.x == 0) {
        // the rectangle: the box of the beam table round the local sensor cell, clipped to the map, grown by R and clipped again
        InflateArgs r = e.rect;
        r.x0 = r.y0 = r.w = r.h = 0;
        if (in) {
            const int bx0 = max(lx + A.min_dx, 0), by0 = max(ly + A.min_dy, 0);
            const int bx1 = min(lx + A.max_dx + 1, nx), by1 = min(ly + A.max_dy + 1, ny);
            if (bx1 > bx0 && by1 > by0) {
                const int gx0 = max(bx0 - r.R, 0), gy0 = max(by0 - r.R, 0), gx1 = min(bx1 + r.R, nx), gy1 = min(by1 + r.R, ny);
                r.x0 = gx0;
                r.y0 = gy0;
                r.w = gx1 - gx0;
                r.h = gy1 - gy0;
            }
        }
        rects[blockIdx.x] = r;
        e.sensor_cell[0] = sx;
        e.sensor_cell[1] = sy;
    }
    if (!in) {   // (the whole workgroup: no barrier is passed)
        for (int r = threadIdx.x; r < n; r += kThreads) e.first[r] = -1;
        return;
    }
    const uint8_t clear = (uint8_t)A.clear_value, mark = (uint8_t)A.mark_value;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, waves = kThreads / kWave;
    // A round is waves * 64 beams, beam base + j * waves + wave the j-th of this wave: lane j fetches it (the slot is host memory:
    // one trip for the wave's 64 beams) and hands it to all lanes when its turn comes.
    for (int base = 0; base < n; base += waves * kWave) {
        const int mine = base + lane * waves + wave;
        int mdx = 0, mdy = 0;
        if (mine < n) {
            mdx = A.beam_xy[2 * (size_t)mine];   // (|dx|, |dy| <= kScanMaxReach: the host's check)
            mdy = A.beam_xy[2 * (size_t)mine + 1];
        }
        const int left = (n - base - wave + waves - 1) / waves, count = left < kWave ? left : kWave;   // this wave's beams of the round
        for (int j = 0; j < count; ++j) {
            const Beam beam(__shfl(mdx, j), __shfl(mdy, j));
            int f = -1;
            if (beam.a != 0) {
                for (unsigned i0 = 0; i0 <= beam.a; i0 += kWave) {
                    const unsigned i = i0 + (unsigned)lane;
                    int wx = 0, wy = 0;
                    bool blocked = false;
                    if (i <= beam.a) {
                        beam.cell(sx, sy, i, wx, wy);
                        if (i >= 1 && wx >= 0 && wx < A.wnx && wy >= 0 && wy < A.wny) blocked = A.world[(size_t)wy * A.wnx + wx] >= A.threshold;
                    }
                    const unsigned long long any = __ballot(blocked);
                    if (any) f = (int)i0 + __ffsll((long long)any) - 1;
                    // the cells of this chunk below the blocked cell, or below the end cell
                    const unsigned stop = f >= 0 ? (unsigned)f : beam.a;
                    if (i < stop) {
                        const int x = wx - e.off_x, y = wy - e.off_y;
                        if (x >= 0 && x < nx && y >= 0 && y < ny) e.layer[(size_t)y * nx + x] = clear;
                    }
                    if (any) break;
                }
            }
            if (lane == 0) {
                const int r = base + j * waves + wave;
                s_first[r] = f;
                e.first[r] = f;
            }
        }
    }
    // every wave's clears have left it, and are visible at workgroup scope, before any wave marks
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const int f = s_first[r];
        if (f < 0) continue;
        const Beam beam(A.beam_xy[2 * (size_t)r], A.beam_xy[2 * (size_t)r + 1]);
        int wx, wy;
        beam.cell(sx, sy, (unsigned)f, wx, wy);
        const int x = wx - e.off_x, y = wy - e.off_y;
        if (x >= 0 && x < nx && y >= 0 && y < ny) e.layer[(size_t)y * nx + x] = mark;
    }
}

}  // namespace

void launch_sense_trace(const SenseEntry* entries, InflateArgs* rects, const int32_t n, const SenseArgs& args, hipStream_t stream) {
    hipLaunchKernelGGL(k_sense_trace, dim3((unsigned)n), dim3(kThreads), 0, stream, entries, rects, args);
}

}  // namespace ccv

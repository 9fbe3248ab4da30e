// The feed kernels of a batch handle (mppi_feed.h): best candidates and optimal paths of every instance.
// Neither is on the tick path; no rollout, prologue or update kernel knows of them.
#include "mppi_feed.h"

#include "fast_trig.h"
#include "mppi_kernels.h"
#include "mppi_select.h"

namespace ccv {

static_assert(kSelectMax == CCV_MPPI_BEST_MAX, "the ABI's limit is the select's");

__global__ __launch_bounds__(kBlock) void k_best_candidates(const BestArgs A) {
    __shared__ SelectShared<kBlock> s;
    const size_t b = blockIdx.x;
    const double* seg = A.cost + b * (size_t)A.kpad;
    select_lowest<kBlock>(seg, A.K, A.N, s);
    for (int j = threadIdx.x; j < A.N; j += kBlock) {
        const int k = s.idx[j];
        A.idx_out[b * A.N + j] = k;
        if (A.cost_out) A.cost_out[b * A.N + j] = seg[k];   // (the cost's own bits: -0.0 and a NaN's payload stay)
    }
    if (!A.xy_out) return;
    // candidate c's row t: (xs, ys)[t][b * kpad + k_c], the layout of k_gather_xy per candidate
    const size_t col0 = b * (size_t)A.kpad;
    double* out = A.xy_out + b * (size_t)A.N * A.H * 2;
    for (int e = threadIdx.x; e < A.N * A.H; e += kBlock) {   // (N * H <= 1024 * 128)
        const int c = e / A.H, t = e - c * A.H;
        const size_t src = (size_t)t * A.pitch + col0 + s.idx[c];
        out[(size_t)e * 2 + 0] = A.xs[src];
        out[(size_t)e * 2 + 1] = A.ys[src];
    }
}

// The plant step is advance_body()'s (mppi_update_device.h), restated here rather than shared: that function is inlined into every
// prologue kernel, and those stay instruction-identical only if nothing about it moves.  Same operations in the same order --
// fast_sincos of the heading, x + v cos dt, y + v sin dt, rebase_angle of the integrated yaw -- as ccv_mppi_plant_step()
// restates them on the host.
__global__ __launch_bounds__(kBlock) void k_optimal_paths(const PathArgs A) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= A.B) return;
    const BatchHead* hd = reinterpret_cast<const BatchHead*>(A.rec + (size_t)b * A.rec_doubles);
    const double dt = hd->dt;
    double x = hd->x0[0], y = hd->x0[1], yaw = hd->x0[2];   // (full body: roll and pitch reach no row of the output)
    const int ud = udim_of(A.model);
    const double* u = A.nominal + (size_t)b * A.R;
    double* out = A.out + (size_t)b * (A.H - 1) * 3;
    for (int i = 0; i < A.H - 1; ++i) {
        out[i * 3 + 0] = x;
        out[i * 3 + 1] = y;
        out[i * 3 + 2] = yaw;
        const double* cmd = u + i * ud;
        const double v = cmd[0], w = cmd[1];
        const double heading = A.model == CCV_MPPI_DIFF_DRIVE ? yaw : yaw + cmd[2];
        double sn, cs;
        fast_sincos(heading, sn, cs);
        x = x + v * cs * dt;
        y = y + v * sn * dt;
        yaw = rebase_angle(yaw + w * dt);
    }
}

}  // namespace ccv

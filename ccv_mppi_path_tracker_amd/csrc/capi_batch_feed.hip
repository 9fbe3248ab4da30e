// C ABI, batch handles: what a node publishes per robot, for all instances at once (ccv_mppi_batch_read_best_candidates,
// ccv_mppi_batch_read_optimal_paths; the kernels: mppi_feed.h).  Each call: its kernel into the handle's scratch, one
// device-to-host copy per output array, one synchronisation; nothing is sorted on the host and nothing goes to the device.
#include "capi_internal.h"
#include "mppi_feed.h"

namespace {

// batch_check_read (capi_batch.hip) for a call that reads every instance, without its flush
int feed_check(ccv_mppi_batch* bh, const void* out) {
    if (!bh || !out) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->have_result) return fail(bh, CCV_MPPI_ERR_STATE, "no iteration yet");
    return CCV_MPPI_OK;
}

}  // namespace

extern "C" {

int ccv_mppi_batch_read_best_candidates(ccv_mppi_batch* bh, int32_t count, int32_t* sample_out, double* cost_out, double* xy_out) {
    if (int rc = feed_check(bh, sample_out)) return rc;
    if (count < 0 || count > bh->K || count > CCV_MPPI_BEST_MAX)
        return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "count < 0, above num_samples or above CCV_MPPI_BEST_MAX");
    if (xy_out && (bh->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE)) return fail(bh, CCV_MPPI_ERR_STATE, "state buffer disabled (NO_STATE_STORE)");
    if (count == 0) return CCV_MPPI_OK;
    // costs and states are the rollout launch's: a pending resident update (it reads the partial sums, writes u*) stays pending
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    // scratch: [B][count] costs | [B][count][H][2] states | [B][count] indices
    const size_t n = (size_t)bh->B * count, n_cost = cost_out ? n : 0, n_xy = xy_out ? n * bh->H * 2 : 0;
    HIP_TRY(bh, ensure_scratch(*bh, (n_cost + n_xy) * sizeof(double) + n * sizeof(int32_t)));
    BestArgs A;
    A.cost = bh->d_cost;
    A.xs = bh->d_xs;
    A.ys = bh->d_ys;
    A.cost_out = cost_out ? bh->d_scratch : nullptr;
    A.xy_out = xy_out ? bh->d_scratch + n_cost : nullptr;
    A.idx_out = reinterpret_cast<int32_t*>(bh->d_scratch + n_cost + n_xy);
    A.K = bh->K;
    A.kpad = bh->kpad;
    A.pitch = bh->pitch;
    A.H = bh->H;
    A.N = count;
    hipLaunchKernelGGL(k_best_candidates, dim3(bh->B), dim3(kBlock), 0, bh->stream, A);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipMemcpyAsync(sample_out, A.idx_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, bh->stream));
    if (cost_out) HIP_TRY(bh, hipMemcpyAsync(cost_out, A.cost_out, n_cost * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    if (xy_out) HIP_TRY(bh, hipMemcpyAsync(xy_out, A.xy_out, n_xy * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_optimal_paths(ccv_mppi_batch* bh, double* xyyaw_out) {
    if (int rc = feed_check(bh, xyyaw_out)) return rc;
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    if (int rc = batch_flush(bh)) return rc;   // (u* of the last tick, as ccv_mppi_batch_get_nominal)
    const size_t n = (size_t)bh->B * (bh->H - 1) * 3;
    HIP_TRY(bh, ensure_scratch(*bh, n * sizeof(double)));
    PathArgs A;
    A.rec = bh->d_rec;
    A.nominal = bh->d_nominal;
    A.out = bh->d_scratch;
    A.B = bh->B;
    A.H = bh->H;
    A.R = bh->R;
    A.model = bh->cfg.model;
    A.rec_doubles = bh->rec_doubles;
    hipLaunchKernelGGL(k_optimal_paths, dim3((bh->B + kBlock - 1) / kBlock), dim3(kBlock), 0, bh->stream, A);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipMemcpyAsync(xyyaw_out, bh->d_scratch, n * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

}  // extern "C"

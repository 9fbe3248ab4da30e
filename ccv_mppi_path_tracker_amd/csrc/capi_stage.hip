// C ABI, one stage at a time (sampling / rollout / weights / update, as the reference's member functions), the read-back
// calls and the timing of the fused iteration.
#include "capi_internal.h"
#include "mppi_top_weights.h"

extern "C" {

// ---- stage-wise -------------------------------------------------------------------------------------------------

int ccv_mppi_sample(ccv_mppi_handle* h, uint64_t seed, uint64_t iter) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    RolloutArgs A;
    const double zero[5] = {0, 0, 0, 0, 0};
    fill_args(h, A, zero, 0.1, 0.0, seed, iter);
    int rc = launch_sample(h, A);
    if (rc) return rc;
    // (no host wait: the stage-wise calls hand nothing back to the host before ccv_mppi_update -- sampling(),
    //  predict_States() and calc_Weights() are void in the reference -- so they only enqueue; the stream keeps their order,
    //  ccv_mppi_update and every read-back wait for what they return)
    for (int d = 0; d < h->udim; ++d) h->inj_absmax[d] = std::fmax(std::fabs(h->cfg.u_min[d]), std::fabs(h->cfg.u_max[d]));
    h->controls_in_z = false;
    h->have_controls = true;
    h->have_rollout = h->have_weights = false;
    return CCV_MPPI_OK;
}

int ccv_mppi_inject_controls(ccv_mppi_handle* h, const double* u_samples) {
    if (!h || !u_samples) return CCV_MPPI_ERR_INVALID_ARG;
    // [K][(H-1)][u_dim] -> rows n = t*u_dim + d of pitch doubles
    std::vector<double> tmp((size_t)h->R * h->pitch, 0.0);
    for (int d = 0; d < CCV_MPPI_MAX_UDIM; ++d) h->inj_absmax[d] = 0.0;
    for (int i = 0; i < h->K; ++i)
        for (int n = 0; n < h->R; ++n) {
            const double v = u_samples[(size_t)i * h->R + n];
            tmp[(size_t)n * h->pitch + i] = v;
            const int d = n % h->udim;
            if (!(std::fabs(v) <= h->inj_absmax[d])) h->inj_absmax[d] = std::fabs(v);   // NaN sticks
        }
    HIP_TRY(h, hipMemcpyAsync(h->d_u, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->controls_in_z = false;
    h->have_controls = true;
    h->have_rollout = h->have_weights = false;
    return CCV_MPPI_OK;
}

int ccv_mppi_rollout(ccv_mppi_handle* h, const double* x0, double dt) {
    if (!h || !x0) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->have_controls) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_rollout before ccv_mppi_sample/inject_controls");
    RolloutArgs A;
    Window W;
    std::memset(&W, 0, sizeof(W));
    fill_args(h, A, x0, dt, 0.0, 0, 0);
    A.store_u = 0;
    A.store_xy = 1;
    A.do_cost = 0;
    int rc = launch_rollout(h, A, W, MODE_ROLLOUT);
    if (rc) return rc;
    std::memcpy(h->st_x0, A.x0, sizeof(h->st_x0));
    h->st_dt = dt;
    h->have_rollout = true;
    h->have_weights = false;
    return CCV_MPPI_OK;
}

int ccv_mppi_weights(ccv_mppi_handle* h, const double* x_ref, const double* y_ref, double yaw_ref0) {
    if (!h || !x_ref || !y_ref) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->have_rollout) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_weights before ccv_mppi_rollout");
    RolloutArgs A;
    Window W;
    fill_args(h, A, h->st_x0, h->st_dt, yaw_ref0, 0, 0);
    window_coeffs(h->H, x_ref, y_ref, h->st_x0[0], h->st_x0[1], W.a, W.b, W.c);
    A.store_u = 0;
    A.store_xy = 0;
    A.do_cost = 1;
    // the rollout is recomputed from the stored controls (bit-identical to the stored states) and scored
    int rc = launch_rollout(h, A, W, MODE_COST);
    if (rc) return rc;
    // sum of weights (calc_Weights normalises, dd:222) without touching u*
    rc = launch_update(h, false, nullptr);
    if (rc) return rc;
    h->have_weights = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_update(ccv_mppi_handle* h, double* u_opt_out, ccv_mppi_stats* stats) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->have_weights) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_update before ccv_mppi_weights");
    h->want_mail = !(stats && h->timing);
    int rc = launch_update(h, true, nullptr);
    h->want_mail = false;
    if (rc) return rc;
    return fetch_result(h, u_opt_out, stats);
}

// ---- read-back --------------------------------------------------------------------------------------------------

int ccv_mppi_read_candidates(ccv_mppi_handle* h, int32_t first, int32_t count, int32_t stride, double* xy_out) {
    if (!h || !xy_out || first < 0 || count < 0 || stride < 1) return CCV_MPPI_ERR_INVALID_ARG;
    if (h->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE) return fail(h, CCV_MPPI_ERR_STATE, "state buffer disabled (NO_STATE_STORE)");
    if (!h->have_rollout) return fail(h, CCV_MPPI_ERR_STATE, "no rollout yet");
    if (count == 0) return CCV_MPPI_OK;
    if ((int64_t)first + (int64_t)(count - 1) * stride >= h->K) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "candidate range exceeds num_samples");
    const size_t n = (size_t)count * h->H * 2;
    HIP_TRY(h, ensure_scratch(*h, n * sizeof(double)));
    hipLaunchKernelGGL(k_gather_xy, dim3((count * h->H + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->d_xs, h->d_ys,
                       h->pitch, h->H, first, count, stride, h->d_scratch);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(xy_out, h->d_scratch, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_read_top_candidates(ccv_mppi_handle* h, int32_t count, int32_t* sample_out, double* weight_out, double* xy_out) {
    if (!h || !sample_out || count < 0) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->have_weights) return fail(h, CCV_MPPI_ERR_STATE, "no weights yet");
    if (count > h->K) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "count exceeds num_samples");
    if (xy_out && (h->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE)) return fail(h, CCV_MPPI_ERR_STATE, "state buffer disabled (NO_STATE_STORE)");
    if (count == 0) return CCV_MPPI_OK;
    // scratch: [count] indices (as 8-byte slots) | [count] weights | [count][H][2] states
    const size_t n_xy = xy_out ? (size_t)count * h->H * 2 : 0;
    HIP_TRY(h, ensure_scratch(*h, ((size_t)count * 2 + n_xy) * sizeof(double)));
    int* d_idx = reinterpret_cast<int*>(h->d_scratch.get());
    double* d_wsel = h->d_scratch + count;
    double* d_xy = h->d_scratch + 2 * (size_t)count;
    hipLaunchKernelGGL(k_top_weights, dim3(1), dim3(kTopBlock), 0, h->stream, h->d_w, h->K, count, d_idx, d_wsel);
    HIP_TRY(h, hipGetLastError());
    std::vector<int> idx(count);
    std::vector<double> wsel(count);
    HIP_TRY(h, hipMemcpyAsync(idx.data(), d_idx, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(wsel.data(), d_wsel, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    top_order_pairs(count, idx.data(), wsel.data());   // NaN weights first, then descending weight; ties by sample index
    for (int i = 0; i < count; ++i) {
        sample_out[i] = idx[i];
        if (weight_out) weight_out[i] = wsel[i];
    }
    if (xy_out) {
        HIP_TRY(h, hipMemcpyAsync(d_idx, idx.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_gather_xy_list, dim3((count * h->H + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->d_xs, h->d_ys,
                           h->pitch, h->H, d_idx, count, d_xy);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(xy_out, d_xy, n_xy * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return CCV_MPPI_OK;
}

static int check_range(ccv_mppi_handle* h, int32_t first, int32_t count, const void* out) {
    if (!h || !out || first < 0 || count < 0) return CCV_MPPI_ERR_INVALID_ARG;
    if ((int64_t)first + count > h->K) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "range exceeds num_samples");
    return CCV_MPPI_OK;
}

int ccv_mppi_read_costs(ccv_mppi_handle* h, int32_t first, int32_t count, double* out) {
    int rc = check_range(h, first, count, out);
    if (rc) return rc;
    if (!h->have_weights) return fail(h, CCV_MPPI_ERR_STATE, "no costs yet");
    HIP_TRY(h, hipMemcpyAsync(out, h->d_cost + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_read_weights(ccv_mppi_handle* h, int32_t first, int32_t count, double* out) {
    int rc = check_range(h, first, count, out);
    if (rc) return rc;
    if (!h->have_weights) return fail(h, CCV_MPPI_ERR_STATE, "no weights yet");
    if (count == 0) return CCV_MPPI_OK;
    if ((rc = flush_pending(h)) != CCV_MPPI_OK) return rc;   // (sum w)
    HIP_TRY(h, ensure_scratch(*h, (size_t)count * sizeof(double)));
    hipLaunchKernelGGL(k_normalise_weights, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->d_w, h->d_stats,
                       first, count, h->d_scratch);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->d_scratch, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_read_controls(ccv_mppi_handle* h, int32_t first, int32_t count, double* out) {
    int rc = check_range(h, first, count, out);
    if (rc) return rc;
    if (!h->have_controls) return fail(h, CCV_MPPI_ERR_STATE, "no controls yet");
    if (count == 0) return CCV_MPPI_OK;
    std::vector<double> tmp((size_t)h->R * count);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->controls_in_z) {
        // the fused iteration kept the normals and the warm start they were drawn around: u = clamp(double(z) * sigma + u*[n]),
        // the samplers' operations (this file is compiled with -ffp-contract=off: a multiply and an add, as on the device)
        std::vector<float> zt((size_t)h->R * count);
        std::vector<double> nom((size_t)h->R);
        HIP_TRY(h, hipMemcpy2D(zt.data(), (size_t)count * sizeof(float), h->d_z + first, (size_t)h->pitch * sizeof(float),
                               (size_t)count * sizeof(float), (size_t)h->R, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(nom.data(), h->d_nom_used, (size_t)h->R * sizeof(double), hipMemcpyDeviceToHost));
        const bool steer_off = h->cfg.model == CCV_MPPI_FULL_BODY && (h->cfg.flags & CCV_MPPI_FLAG_STEER_OFF);
        for (int n = 0; n < h->R; ++n) {
            const int d = n % h->udim;
            const double lo = h->cfg.u_min[d], hi = h->cfg.u_max[d], sigma = h->cfg.control_noise;
            for (int i = 0; i < count; ++i) {
                const double prod = (double)zt[(size_t)n * count + i] * sigma;
                double v = prod + nom[n];
                v = v < lo ? lo : (v > hi ? hi : v);
                if (steer_off && d == 2) v = 0.0;
                tmp[(size_t)n * count + i] = v;
            }
        }
    } else
    HIP_TRY(h, hipMemcpy2D(tmp.data(), (size_t)count * sizeof(double), h->d_u + first, (size_t)h->pitch * sizeof(double),
                           (size_t)count * sizeof(double), (size_t)h->R, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i)
        for (int n = 0; n < h->R; ++n) out[(size_t)i * h->R + n] = tmp[(size_t)n * count + i];
    return CCV_MPPI_OK;
}


#if defined(CCV_DIAG)
// diagnostic builds: the stamps of the first `nblocks` workgroups of the last launch, kDiagSlots values each (mppi_diag.h)
extern "C" int ccv_mppi_debug_blocks(ccv_mppi_handle* h, unsigned long long* out, int nblocks) {
    if (!h || !out || nblocks < 0 || nblocks > kDiagBlocks) return CCV_MPPI_ERR_INVALID_ARG;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, h->d_dbg + kDiagHeader, (size_t)nblocks * kDiagSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}
#endif

// ---- measurement ------------------------------------------------------------------------------------------------

int ccv_mppi_timing_enable(ccv_mppi_handle* h, int32_t on) { return h ? timing_enable(h, on) : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_timing_read(ccv_mppi_handle* h, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters, int32_t reset) {
    return h ? timing_read(h, rollout_us_sum, iter_us_sum, n_iters, reset) : CCV_MPPI_ERR_INVALID_ARG;
}

int ccv_mppi_batch_timing_enable(ccv_mppi_batch* bh, int32_t on) { return bh ? timing_enable(bh, on) : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_batch_timing_read(ccv_mppi_batch* bh, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters, int32_t reset) {
    return bh ? timing_read(bh, rollout_us_sum, iter_us_sum, n_iters, reset) : CCV_MPPI_ERR_INVALID_ARG;
}

}  // extern "C"

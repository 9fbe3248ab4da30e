// C ABI, batch handles: B independent problems in one launch (ccv_mppi_batch_*; struct ccv_mppi_batch: capi_internal.h) -- what
// a tick runs and what reads its results, the device-resident closed loop included; what configures the next launch is in
// capi_batch_config.hip.  The plumbing is the single handle's (ccv_mppi_capi.hip), on the core.
#include <new>

#include "capi_internal.h"

namespace {

// CCV_MPPI_BATCH_KERNEL_* of a launch (ccv_mppi_batch_last_kernel): every rung up to the plan's sets its bit
int batch_kernel_code(const RolloutPlan& p) {
    const int family = p.family == KernelFamily::Plain     ? CCV_MPPI_BATCH_KERNEL_PLAIN
                       : p.family == KernelFamily::OneWave ? CCV_MPPI_BATCH_KERNEL_ONE_WAVE
                                                           : CCV_MPPI_BATCH_KERNEL_FOUR_WAVE;
    return family | (p.wide ? CCV_MPPI_BATCH_KERNEL_WIDE : 0) | (p.form >= BatchForm::Varied ? CCV_MPPI_BATCH_KERNEL_VARIED : 0) |
           (p.shift ? CCV_MPPI_BATCH_KERNEL_SHIFT : 0) | (p.form >= BatchForm::Obst ? CCV_MPPI_BATCH_KERNEL_OBST : 0) |
           (p.form >= BatchForm::Moving ? CCV_MPPI_BATCH_KERNEL_MOVING : 0) | (p.form >= BatchForm::Grid ? CCV_MPPI_BATCH_KERNEL_GRID : 0);
}

int batch_check_args(ccv_mppi_batch* bh, const double* x0, const double* dt, const double* x_ref, const double* y_ref,
                     const double* yaw_ref0, const uint64_t* seed) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!x0 || !dt || !x_ref || !y_ref || !yaw_ref0 || !seed) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    for (int b = 0; b < bh->B; ++b)
        if (!(dt[b] == dt[b])) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "dt is NaN");
    return CCV_MPPI_OK;
}

int batch_launch(ccv_mppi_batch* bh, RolloutArgs& A, int trig, bool defer);

// fast_trig_safe of instance b (its own clamp bounds), folded into the batch's: the worst instance decides
int batch_trig(const ccv_mppi_batch* bh, const int b, const RolloutArgs& A, const int trig) {
    const int t = fast_trig_safe(bh, batch_cfg(bh, b), A, MODE_FUSED, has_wide_form(*bh, MODE_FUSED));
    return t == kTrigUnsafe || trig == kTrigUnsafe ? kTrigUnsafe : t == kTrigWide ? kTrigWide : trig;
}

// records -> device, rollout of all instances, per-instance update.  The kernel family is the single handle's rule applied to
// the batch's total number of workgroups (chosen at create); the plain kernel for the whole batch when one instance's
// headings can leave the fast sin / cos's range, the wide-turn instantiation when one instance needs it.
int batch_enqueue(ccv_mppi_batch* bh, const double* x0, const double* dt, const double* x_ref, const double* y_ref,
                  const double* yaw_ref0, const uint64_t* seed, uint64_t iter) {
    const int B = bh->B, H = bh->H, nx = bh->cfg.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    Slot slot;
    HIP_TRY(bh, bh->rec_ring.take(slot));
    double* rec = reinterpret_cast<double*>(slot.host);
    std::memset(rec, 0, (size_t)B * bh->rec_doubles * sizeof(double));
    RolloutArgs A;
    fill_args(bh, A, x0, dt[0], yaw_ref0[0], seed[0], iter);
    int trig = bh->fused == KernelFamily::Plain ? kTrigUnsafe : kTrigSafe;
    for (int b = 0; b < B; ++b) {
        const double* xb = x0 + (size_t)5 * b;
        BatchHead* hd = reinterpret_cast<BatchHead*>(rec + (size_t)b * bh->rec_doubles);
        for (int i = 0; i < nx; ++i) hd->x0[i] = xb[i];
        hd->yaw_ref0 = yaw_ref0[b];
        hd->dt = dt[b];
        hd->inv_dt = 1.0 / dt[b];
        hd->seed_lo = (uint32_t)seed[b];
        hd->seed_hi = (uint32_t)(seed[b] >> 32);
        hd->K = b * bh->kpad + bh->K;
        hd->k_offset = -b * bh->kpad;
        hd->nominal = bh->d_nominal + (size_t)b * bh->R;
        if (uses_table(bh)) hd->params = bh->d_params + b;
        double* win = rec + (size_t)b * bh->rec_doubles + kBatchHeadDoubles;
        window_coeffs(H, x_ref + (size_t)b * H, y_ref + (size_t)b * H, hd->x0[0], hd->x0[1], win, win + H, win + 2 * H);
        if (trig != kTrigUnsafe) {
            for (int i = 0; i < 5; ++i) A.x0[i] = hd->x0[i];
            A.dt = dt[b];
            trig = batch_trig(bh, b, A, trig);
        }
    }
    HIP_TRY(bh, bh->rec_ring.seal(slot, hipMemcpyAsync(bh->d_rec, rec, (size_t)B * bh->rec_doubles * sizeof(double), hipMemcpyHostToDevice, bh->stream),
                                  bh->stream));
    return batch_launch(bh, A, trig, false);
}

// the rollout of every instance from the records in d_rec, then the per-instance update; `defer` (resident ticks): the update
// of the fused kernels waits in bh->fin for the next tick's prologue (k_finalize_advance_batch) or for batch_flush
int batch_launch(ccv_mppi_batch* bh, RolloutArgs& A, const int trig, const bool defer) {
    const int B = bh->B;
    const RolloutPlan plan = make_plan(*bh, bh->cfg.model, MODE_FUSED, trig, B, batch_form(bh), bh->min_shift);
    const bool plain = plan.family == KernelFamily::Plain;
    A.frame = reinterpret_cast<const ResidentFrame*>(bh->d_rec.get());
    A.nparts = B * bh->nblocks;   // (partials [(R+1)][B * nblocks]: column = workgroup)
    A.fuse_update = plain ? 0 : 1;
    A.store_u = 1;
    A.store_xy = (bh->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE) ? 0 : 1;
    A.do_cost = 1;
    HIP_TRY(bh, timing_begin(*bh));
    static const Window kNoWindow{};   // (the windows are in the records)
    LaunchAt at;
    HIP_TRY(bh, timing_rollout_at(*bh, bh->stream, plain, at));
    launch_rollout(plan, at, A, kNoWindow);
    HIP_TRY(bh, timing_rollout_done(*bh, bh->stream, plain));
    bh->last_kernel = batch_kernel_code(plan);
    HIP_TRY(bh, hipGetLastError());
    int nparts = bh->nblocks;
    const bool shift = plan.shift && !plain;   // (the update over block-relative partials)
    if (plain) {   // the plain kernel stores w and the controls: the single handle's unfused reduction, instance by instance
        if (plan.shift) {   // ... over weights re-formed around every instance's exact minimum cost (the single handle's MIN_SHIFT)
            if (!bh->d_cmin) HIP_TRY(bh, bh->d_cmin.alloc((size_t)B));
            hipLaunchKernelGGL(k_min_cost_batch, dim3(B), dim3(1024), 0, bh->stream, bh->d_cost, bh->K, bh->kpad, bh->d_cmin);
            hipLaunchKernelGGL(k_reweight_batch, dim3((bh->K + kBlock - 1) / kBlock, B), dim3(kBlock), 0, bh->stream, bh->d_cost,
                               bh->d_cmin, bh->d_params, bh->K, bh->kpad, bh->d_w);
        }
        hipLaunchKernelGGL(k_update_partials_batch, dim3(bh->nchunks, bh->R + 1, B), dim3(kBlock), 0, bh->stream, update_args(bh), bh->kpad);
        nparts = bh->nchunks;
    }
    FinalizeArgs F = finalize_args(bh, bh->d_vec, nparts, true);
    // The mailbox up to the largest one a single handle posts; beyond, one copy and a stream synchronisation are faster
    // (diff drive K = 1 000, H = 15, blocking us, mailbox vs copy, one box: B = 1 45 vs 51, B = 64 107 vs 66, B = 256 220 vs
    // 118; the mailbox_blocking_us / copy_blocking_us columns of profiles/batch_bench.json repeat the comparison)
    const bool mail_fits = (size_t)B * (bh->R + 4) <= (size_t)(CCV_MPPI_MAX_HORIZON - 1) * CCV_MPPI_MAX_UDIM + 4;
    if (bh->want_mail && bh->use_mail && (mail_fits || bh->mail_any_size)) post_to_mail(*bh, F);
    bh->want_mail = false;
    bh->shift_result = shift;
    const UpdatePlan up{F, B, !plain, shift ? bh->d_params : nullptr, bh->K};
    if (defer && !plain && !bh->timed_now && !F.mail) {
        bh->fin = up;
        bh->fin_pending = true;
    } else {
        launch_finalize(*bh, up);
        HIP_TRY(bh, hipGetLastError());
    }
    HIP_TRY(bh, timing_end(*bh, bh->stream));
    HIP_TRY(bh, throttle_tick(*bh, bh->stream));
    bh->have_result = true;
    return CCV_MPPI_OK;
}

// u* [B][R] and the statistics of every instance: from the mailbox the update kernel posted into, or copied
int batch_fetch(ccv_mppi_batch* bh, double* u_opt_out, ccv_mppi_stats* stats) {
    const size_t B = (size_t)bh->B, R = (size_t)bh->R;
    double* v = bh->h_pin;   // [B][R + 4]
    if (bh->mail_pending) {
        bh->mail_pending = false;
        if (int rc = read_mail(bh, B * (R + 4), v)) return rc;
    } else {
        double* u = v + B * (R + 4);
        double* st = u + B * R;
        HIP_TRY(bh, hipMemcpyAsync(u, bh->d_nominal, B * R * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
        HIP_TRY(bh, hipMemcpyAsync(st, bh->d_stats, B * 4 * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
        HIP_TRY(bh, hipStreamSynchronize(bh->stream));
        for (size_t b = 0; b < B; ++b) {
            std::memcpy(v + b * (R + 4), u + b * R, R * sizeof(double));
            std::memcpy(v + b * (R + 4) + R, st + b * 4, 4 * sizeof(double));
        }
    }
    if (stats && bh->timing) HIP_TRY(bh, timing_collect(*bh, bh->stream));
    for (size_t b = 0; b < B; ++b)
        unpack_result(*bh, bh->R, v + b * (R + 4), u_opt_out ? u_opt_out + b * R : nullptr, stats ? stats + b : nullptr);
    return CCV_MPPI_OK;
}

// the fleet's lists exist only where the poses live: the host-record calls are refused while the term is on
const char kFleetHostRecord[] = "the fleet term is on: resident steps only (ccv_mppi_batch_resident_set_fleet)";

int batch_check_read(ccv_mppi_batch* bh, int32_t instance, const void* out) {
    if (!bh || !out) return CCV_MPPI_ERR_INVALID_ARG;
    if (instance < 0 || instance >= bh->B) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "instance out of range");
    if (!bh->have_result) return fail(bh, CCV_MPPI_ERR_STATE, "no iteration yet");
    return batch_flush(bh);
}
}  // namespace

extern "C" {

int ccv_mppi_batch_create(const ccv_mppi_config* cfg, int32_t batch, ccv_mppi_batch** out) {
    // every argument is checked before a device is looked at
    if (!cfg || !out) return CCV_MPPI_ERR_INVALID_ARG;
    *out = nullptr;
    if (int rc = check_config(cfg)) return rc;
    if (cfg->sample_offset != 0) return CCV_MPPI_ERR_INVALID_ARG;
    if (cfg->flags & CCV_MPPI_FLAG_MIN_SHIFT) return CCV_MPPI_ERR_INVALID_ARG;
    if (batch < 1) return CCV_MPPI_ERR_INVALID_ARG;
    const int kpad = round_up(cfg->num_samples, 64);
    if ((int64_t)batch * kpad > (int64_t)CCV_MPPI_BATCH_MAX_SAMPLES) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = check_device(cfg->device)) return rc;
    ccv_mppi_batch* bh = new (std::nothrow) ccv_mppi_batch();
    if (!bh) return CCV_MPPI_ERR_ALLOC;
    const DeviceGuard guard(cfg->device);
    set_shape(*bh, *cfg, /*pitch=*/batch * kpad, /*workgroups per instance=*/kpad / kPcSamples);
    bh->B = batch;
    bh->kpad = kpad;
    bh->rec_doubles = batch_record_doubles(bh->H);
    // the single handle's selection on the batch's workgroups; CCV_MPPI_KERNEL=v1 selects the plain kernel, its other values
    // and CCV_MPPI_WINDOW / _PRIO / _PRUNE / _FAST_CLAMP are ignored here
    select_kernels(*bh, *bh, (int64_t)batch * bh->nblocks, /*batched=*/true);

    auto bail = [&](int code) {
        std::fprintf(stderr, "ccv_mppi_batch_create: %s\n", bh->err.c_str());
        ccv_mppi_batch_destroy(bh);
        return code;
    };
    hipError_t e;
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail(fail(bh, CCV_MPPI_ERR_NO_DEVICE, "hipSetDevice", e));
    const size_t B = (size_t)batch, R = (size_t)bh->R;
    const size_t nparts_max = B * (size_t)(bh->nblocks > bh->nchunks ? bh->nblocks : bh->nchunks);
    const size_t pad = (size_t)(CCV_MPPI_MAX_HORIZON + 8) * CCV_MPPI_MAX_UDIM;   // (u* is read 4 at a time)
    // (pinned staging: the mailbox's values, or the two copies of the fall-back path)
    if (int rc = create_buffers(bh, BufferCounts{nparts_max, /*nominal=*/B * R + pad, /*vec=*/B * (R + 1), /*stats=*/B * 4, &bh->d_rec,
                                                B * bh->rec_doubles, /*pin_doubles=*/B * (R + 4) * 2, /*mail_slots=*/B * (R + 4)}))
        return bail(rc);
    if ((e = bh->rec_ring.create(ccv_mppi_batch::kRecSlots, B * bh->rec_doubles * sizeof(double), /*mapped=*/false)) != hipSuccess)
        return bail(fail(bh, CCV_MPPI_ERR_ALLOC, "hipHostMalloc", e));
    if (const char* mv = std::getenv("CCV_MPPI_BATCH_MAIL")) bh->mail_any_size = std::strcmp(mv, "1") == 0;
    *out = bh;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_destroy(ccv_mppi_batch* bh) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const DeviceGuard guard(bh->cfg.device);
    (void)hipSetDevice(bh->cfg.device);
    if (bh->stream) (void)batch_flush(bh);
    wait_for_streams(bh);
    delete bh;
    return CCV_MPPI_OK;
}

const char* ccv_mppi_batch_last_error(const ccv_mppi_batch* bh) { return bh ? bh->err.c_str() : "null handle"; }

int ccv_mppi_batch_size(const ccv_mppi_batch* bh) { return bh ? bh->B : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_batch_last_kernel(const ccv_mppi_batch* bh) { return bh ? bh->last_kernel : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_batch_set_stream(ccv_mppi_batch* bh, void* hip_stream) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = batch_flush(bh)) return rc;
    return set_stream(bh, hip_stream);
}

int ccv_mppi_batch_synchronize(ccv_mppi_batch* bh) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_set_nominal(ccv_mppi_batch* bh, const double* u) {
    if (!bh || !u) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = batch_flush(bh)) return rc;   // (a deferred resident update must not land on top of it)
    HIP_TRY(bh, hipMemcpyAsync(bh->d_nominal, u, (size_t)bh->B * bh->R * sizeof(double), hipMemcpyHostToDevice, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    track_absmax(u, (size_t)bh->B * bh->R, bh->udim, bh->nom_absmax);
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_get_nominal(ccv_mppi_batch* bh, double* u) {
    if (!bh || !u) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipMemcpyAsync(u, bh->d_nominal, (size_t)bh->B * bh->R * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_iterate(ccv_mppi_batch* bh, const double* x0, const double* dt, const double* x_ref, const double* y_ref,
                           const double* yaw_ref0, const uint64_t* seed, uint64_t iter, double* u_opt_out, ccv_mppi_stats* stats) {
    int rc = batch_check_args(bh, x0, dt, x_ref, y_ref, yaw_ref0, seed);
    if (rc) return rc;
    if (bh->fleet) return fail(bh, CCV_MPPI_ERR_STATE, kFleetHostRecord);
    if ((rc = batch_flush(bh))) return rc;   // (the rollout reads u*)
    bh->want_mail = !(stats && bh->timing);   // (a timed call synchronises for its events anyway)
    rc = batch_enqueue(bh, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter);
    bh->want_mail = false;
    if (rc) return rc;
    return batch_fetch(bh, u_opt_out, stats);
}

int ccv_mppi_batch_iterate_enqueue(ccv_mppi_batch* bh, const double* x0, const double* dt, const double* x_ref,
                                   const double* y_ref, const double* yaw_ref0, const uint64_t* seed, uint64_t iter) {
    int rc = batch_check_args(bh, x0, dt, x_ref, y_ref, yaw_ref0, seed);
    if (rc) return rc;
    if (bh->fleet) return fail(bh, CCV_MPPI_ERR_STATE, kFleetHostRecord);
    if ((rc = batch_flush(bh))) return rc;   // (the rollout reads u*)
    return batch_enqueue(bh, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter);
}

int ccv_mppi_batch_read_costs(ccv_mppi_batch* bh, int32_t instance, int32_t first, int32_t count, double* out) {
    if (int rc = batch_check_read(bh, instance, out)) return rc;
    if (first < 0 || count < 0 || (int64_t)first + count > bh->K) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "range exceeds num_samples");
    const size_t col = (size_t)instance * bh->kpad + first;
    HIP_TRY(bh, hipMemcpyAsync(out, bh->d_cost + col, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_weights(ccv_mppi_batch* bh, int32_t instance, int32_t first, int32_t count, double* out) {
    if (int rc = batch_check_read(bh, instance, out)) return rc;
    if (first < 0 || count < 0 || (int64_t)first + count > bh->K) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "range exceeds num_samples");
    if (count == 0) return CCV_MPPI_OK;
    HIP_TRY(bh, ensure_scratch(*bh, (size_t)count * sizeof(double)));
    const dim3 grid((count + kBlock - 1) / kBlock);
    if (bh->shift_result)   // (the last launch left block-relative weights: the SHIFT rollout kernels)
        hipLaunchKernelGGL(k_normalise_weights_shift, grid, dim3(kBlock), 0, bh->stream, bh->d_w + (size_t)instance * bh->kpad,
                           bh->d_statpart + (size_t)instance * bh->nblocks * 3, bh->d_stats + (size_t)instance * 4,
                           batch_cfg(bh, instance).lambda, first, count, bh->d_scratch);
    else
        hipLaunchKernelGGL(k_normalise_weights, grid, dim3(kBlock), 0, bh->stream, bh->d_w + (size_t)instance * bh->kpad,
                           bh->d_stats + (size_t)instance * 4, first, count, bh->d_scratch);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipMemcpyAsync(out, bh->d_scratch, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_candidates(ccv_mppi_batch* bh, int32_t instance, int32_t first, int32_t count, int32_t stride,
                                   double* xy_out) {
    if (int rc = batch_check_read(bh, instance, xy_out)) return rc;
    if (first < 0 || count < 0 || stride < 1) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "first < 0, count < 0 or stride < 1");
    if (bh->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE) return fail(bh, CCV_MPPI_ERR_STATE, "state buffer disabled (NO_STATE_STORE)");
    if (count == 0) return CCV_MPPI_OK;
    if ((int64_t)first + (int64_t)(count - 1) * stride >= bh->K) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "candidate range exceeds num_samples");
    const size_t n = (size_t)count * bh->H * 2;
    HIP_TRY(bh, ensure_scratch(*bh, n * sizeof(double)));
    hipLaunchKernelGGL(k_gather_xy, dim3((count * bh->H + kBlock - 1) / kBlock), dim3(kBlock), 0, bh->stream, bh->d_xs, bh->d_ys,
                       bh->pitch, bh->H, instance * bh->kpad + first, count, stride, bh->d_scratch);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipMemcpyAsync(xy_out, bh->d_scratch, n * sizeof(double), hipMemcpyDeviceToHost, bh->stream));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

// ---- batch handles: device-resident closed loop of every instance (mppi_resident.h) ---------------------------------

int ccv_mppi_batch_resident_set_paths(ccv_mppi_batch* bh, const double* path_x, const double* path_y, const int32_t* n_path,
                                      const double* resolution) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!path_x || !path_y || !n_path || !resolution) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const int B = bh->B;
    std::vector<BatchInstance> inst((size_t)B);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (n_path[b] < 1 || !(resolution[b] > 0.0))
            return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "paths: an empty path or a resolution <= 0");
        inst[b] = BatchInstance{};
        inst[b].path_off = total;
        inst[b].n_path = n_path[b];
        inst[b].resolution = resolution[b];
        if (bh->inst.size() == (size_t)B) {   // (the noise keys of ccv_mppi_batch_resident_set_poses stay)
            inst[b].seed_lo = bh->inst[b].seed_lo;
            inst[b].seed_hi = bh->inst[b].seed_hi;
        }
        total += n_path[b];
    }
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (a queued prologue may still read the old paths)
    // every allocation comes before anything is dropped: a longer set gets a new path array (a shorter one reuses the present
    // one), the first call the frames, the instances and the traces
    DeviceArray<double> path, trace;
    DeviceArray<ResidentFrame> frames;
    DeviceArray<BatchInstance> rows;
    const bool grow = total > bh->n_total || !bh->d_rpath, first = !bh->d_rframe;
    if (grow) HIP_TRY(bh, path.alloc((size_t)2 * total));
    const size_t trace_doubles = (size_t)B * CCV_MPPI_BATCH_TRACE_ROWS * 6;
    if (first) {
        HIP_TRY(bh, frames.alloc((size_t)B));
        HIP_TRY(bh, rows.alloc((size_t)B));
        HIP_TRY(bh, trace.alloc(trace_doubles));
    }
    double* const to = grow ? path.get() : bh->d_rpath.get();
    HIP_TRY(bh, hipMemcpy(to, path_x, (size_t)total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(bh, hipMemcpy(to + total, path_y, (size_t)total * sizeof(double), hipMemcpyHostToDevice));
    if (first) {
        HIP_TRY(bh, hipMemset(frames, 0, (size_t)B * sizeof(ResidentFrame)));
        HIP_TRY(bh, hipMemset(trace, 0, trace_doubles * sizeof(double)));
    }
    HIP_TRY(bh, hipMemcpy(first ? rows.get() : bh->d_inst.get(), inst.data(), (size_t)B * sizeof(BatchInstance), hipMemcpyHostToDevice));
    // commit: nothing below fails
    bh->drop_plan();   // (the paths are the caller's again: ccv_mppi_batch_resident_set_plan comes after this call)
    if (grow) bh->d_rpath = std::move(path);
    if (first) {
        bh->d_rframe = std::move(frames);
        bh->d_inst = std::move(rows);
        bh->d_rtrace = std::move(trace);
    }
    bh->n_total = total;   // (the y half starts at n_total)
    bh->inst.swap(inst);
    bh->have_paths = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_set_poses(ccv_mppi_batch* bh, const double* state, const uint64_t* seed) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!state || !seed) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->have_paths) return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_paths first");
    const int B = bh->B, nx = bh->cfg.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    std::vector<FrameHead> heads((size_t)B);   // (as ccv_mppi_resident_set_pose)
    std::vector<double> angles((size_t)B * 3);
    for (int b = 0; b < B; ++b) {
        heads[b] = FrameHead{};
        for (int i = 0; i < nx; ++i) heads[b].x0[i] = state[(size_t)b * 5 + i];
        for (int i = 0; i < 3; ++i) angles[(size_t)b * 3 + i] = std::fabs(heads[b].x0[2 + i]);
        bh->inst[b].seed_lo = (uint32_t)seed[b];
        bh->inst[b].seed_hi = (uint32_t)(seed[b] >> 32);
    }
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    HIP_TRY(bh, hipMemcpy2D(bh->d_rframe, sizeof(ResidentFrame), heads.data(), sizeof(FrameHead), sizeof(FrameHead), (size_t)B,
                           hipMemcpyHostToDevice));
    if (bh->plan)   // (the device's n_path is the truth while planning is set: the noise keys alone go up)
        HIP_TRY(bh, hipMemcpy2D(&bh->d_inst.get()->seed_lo, sizeof(BatchInstance), &bh->inst[0].seed_lo, sizeof(BatchInstance), 2 * sizeof(uint32_t),
                               (size_t)B, hipMemcpyHostToDevice));
    else HIP_TRY(bh, hipMemcpy(bh->d_inst, bh->inst.data(), (size_t)B * sizeof(BatchInstance), hipMemcpyHostToDevice));
    if (bh->fleet) {
        std::vector<double> xy((size_t)B * 2);
        for (int b = 0; b < B; ++b) std::memcpy(&xy[(size_t)b * 2], heads[b].x0, 2 * sizeof(double));
        if (int rc = fleet_restart(bh, xy.data())) return rc;
    }
    bh->res_angle_abs.swap(angles);
    bh->res_steps = 0;
    bh->have_poses = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_step_enqueue(ccv_mppi_batch* bh, double dt, uint64_t iter, int32_t advance) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const ccv_mppi_config& c = bh->cfg;
    const int B = bh->B;
    // every check that can refuse the step comes before anything is launched: no pose moves on a refusal
    if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "resident step: dt must be finite and not negative");
    if (!bh->have_paths || !bh->have_poses)
        return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_paths and _set_poses first");
    for (int b = 0; b < B; ++b) {
        const double stride = batch_cfg(bh, b).v_ref * dt / bh->inst[b].resolution;   // (the instance's own v_ref)
        if (!std::isfinite(stride) || stride < 0.0 || stride * bh->H > 2.0e9)
            return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "resident step: v_ref * dt / resolution is not a usable window stride");
    }
    // the angle bounds of a single handle's resident step (resident_bounds), instance by instance and with the instance's own
    // clamp bounds; the batch's kernel rule (select_kernels) with no plain kernel: the wide-turn instantiation when one
    // instance needs it, a refusal where the plain kernel would be needed
    std::vector<double> nb(bh->res_angle_abs);
    int trig = bh->fused == KernelFamily::Plain ? kTrigUnsafe : kTrigSafe;
    RolloutArgs A;
    const double zero[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    fill_args(bh, A, zero, dt, 0.0, 0, iter);   // (the instance's pose, window and key: its record, batch_view)
    for (int b = 0; b < B && trig != kTrigUnsafe; ++b) {
        const ResidentBounds r = resident_bounds(*bh, batch_cfg(bh, b), bh->res_angle_abs.data() + (size_t)b * 3, dt, advance);
        for (int i = 0; i < 3; ++i) A.x0[2 + i] = nb[(size_t)b * 3 + i] = r.angle[i];
        trig = r.heading <= kFastTrigLimit ? batch_trig(bh, b, A, trig) : kTrigUnsafe;
    }
    if (trig == kTrigUnsafe)
        return fail(bh, CCV_MPPI_ERR_STATE, "the resident loop needs the cooperative kernels and bounded pose angles / commands");
    BatchAdvanceArgs G;
    G.frames = bh->d_rframe;
    G.rec = bh->d_rec;
    G.inst = bh->d_inst;
    G.path = bh->d_rpath;
    G.nominal = bh->d_nominal;
    G.trace = bh->d_rtrace;
    G.n_total = bh->n_total;
    G.dt = dt;
    G.inv_dt = 1.0 / dt;
    G.v_ref = c.v_ref;
    G.H = bh->H;
    G.R = bh->R;
    G.K = bh->K;
    G.kpad = bh->kpad;
    G.model = c.model;
    G.advance = advance ? 1 : 0;
    G.trace_cap = CCV_MPPI_BATCH_TRACE_ROWS;
    // the fleet term: this tick's snapshot is half res_steps & 1 of the position table, the prologue writes the other
    FleetArgs L{};
    if (bh->fleet) {
        const size_t half = (size_t)B * 2;
        L.xy_in = bh->d_fleet_xy + (size_t)(bh->res_steps & 1) * half;
        L.xy_out = bh->d_fleet_xy + (size_t)((bh->res_steps + 1) & 1) * half;
        L.radius = bh->d_fleet_radius;
        L.n_static = bh->d_fleet_nstatic;
        L.obst = bh->d_obst;
        L.range2 = bh->fleet_range * bh->fleet_range;
        L.max_neighbours = bh->fleet_maxn;
        L.B = B;
    }
    FleetPredArgs V{};
    const bool pred = bh->fleet && bh->fleet_pred;
    if (pred) {
        const size_t half = (size_t)B * 2;
        V.v_in = bh->d_fleet_v + (size_t)(bh->res_steps & 1) * half;
        V.v_out = bh->d_fleet_v + (size_t)((bh->res_steps + 1) & 1) * half;
        V.obst_v = bh->d_obst_v;
    }
    // (varied: the prologue takes each instance's v_ref from the parameter table and points its record's head at its row)
    if (bh->fin_pending) {   // the last tick's update and this tick's prologue: one launch
        launch_finalize_advance(*bh, bh->fin, G, uses_table(bh) ? bh->d_params : nullptr, bh->fleet ? &L : nullptr, pred ? &V : nullptr);
        bh->fin_pending = false;
    } else {
        if (pred) hipLaunchKernelGGL(k_advance_batch_fleet_pred, dim3(B), dim3(kBatchAdvanceThreads), 0, bh->stream, G, bh->d_params, L, V);
        else if (bh->fleet) hipLaunchKernelGGL(k_advance_batch_fleet, dim3(B), dim3(kBatchAdvanceThreads), 0, bh->stream, G, bh->d_params, L);
        else if (uses_table(bh)) hipLaunchKernelGGL(k_advance_batch_varied, dim3(B), dim3(kBatchAdvanceThreads), 0, bh->stream, G, bh->d_params);
        else hipLaunchKernelGGL(k_advance_batch, dim3(B), dim3(kBatchAdvanceThreads), 0, bh->stream, G);
    }
    HIP_TRY(bh, hipGetLastError());
    bh->res_steps += 1;
    bh->res_angle_abs.swap(nb);
    // the rollout reads every instance's record (batch_view): pose, window, dt, noise key, warm start
    A.frame = reinterpret_cast<const ResidentFrame*>(bh->d_rec.get());
    return batch_launch(bh, A, trig, true);
}

int ccv_mppi_batch_resident_read(ccv_mppi_batch* bh, double* state, int32_t* current_index, double* x_ref, double* y_ref,
                                 double* yaw_ref0, int64_t* steps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->have_paths || !bh->have_poses)
        return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_paths and _set_poses first");
    const int B = bh->B, H = bh->H, nx = bh->cfg.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    std::vector<ResidentFrame> F((size_t)B);
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    HIP_TRY(bh, hipMemcpy(F.data(), bh->d_rframe, (size_t)B * sizeof(ResidentFrame), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        if (state) {
            for (int i = 0; i < 5; ++i) state[(size_t)b * 5 + i] = i < nx ? F[b].x0[i] : 0.0;
        }
        if (current_index) current_index[b] = F[b].index;
        if (x_ref) std::memcpy(x_ref + (size_t)b * H, F[b].x_ref, (size_t)H * sizeof(double));
        if (y_ref) std::memcpy(y_ref + (size_t)b * H, F[b].y_ref, (size_t)H * sizeof(double));
        if (yaw_ref0) yaw_ref0[b] = F[b].yaw_ref0;
    }
    if (steps) *steps = bh->res_steps;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_trace(ccv_mppi_batch* bh, int32_t instance, int32_t max_rows, double* rows, int32_t* n_rows) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!rows || !n_rows || max_rows < 0) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "rows / n_rows null or max_rows < 0");
    if (instance < 0 || instance >= bh->B) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "instance out of range");
    if (!bh->have_paths || !bh->have_poses)
        return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_paths and _set_poses first");
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    const int64_t cap = CCV_MPPI_BATCH_TRACE_ROWS;
    HIP_TRY(bh, read_trace_ring(bh->d_rtrace + (size_t)instance * cap * 6, cap, bh->res_steps, max_rows, rows, n_rows));
    return CCV_MPPI_OK;
}

}  // extern "C"

// C ABI (include/ccv_mppi.h) over the gfx950 rollout kernels (mppi_rollout_*.h, launched through mppi_launch.h; their shared
// vocabulary: mppi_kernels.h).
// Host side only orchestrates: allocate once, build the window coefficients, launch, copy u* back.
// There is deliberately no CPU fallback: every entry point fails with CCV_MPPI_ERR_NO_DEVICE / _HIP.
// The other host units (capi_internal.h lists them) call the plumbing defined here.
#include <chrono>
#include <new>

#include "capi_internal.h"

namespace ccv {

hipError_t ensure_scratch(DeviceBuffers& d, size_t bytes) {
    if (bytes <= d.scratch_bytes) return hipSuccess;
    d.d_scratch.reset();
    d.scratch_bytes = 0;
    if (hipError_t e = d.d_scratch.alloc((bytes + sizeof(double) - 1) / sizeof(double))) return e;
    d.scratch_bytes = bytes;
    return hipSuccess;
}

// the controller parameters of configuration c (sigma, lambda, v_ref, bounds, clamp form, weights) into A: fill_args(), and
// every row of a batch's parameter table (batch_params_of)
void fill_params(const ccv_mppi_config& c, const bool fast_clamp_allowed, RolloutArgs& A) {
    A.sigma = c.control_noise;
    A.lambda = c.lambda;
    A.v_ref = c.v_ref;
    for (int d = 0; d < CCV_MPPI_MAX_UDIM; ++d) {
        A.umin[d] = c.u_min[d];
        A.umax[d] = c.u_max[d];
    }
    // two-instruction clamps (clampd_fast, mppi_device_util.h) give the reference's values when no control is NaN and no pair of
    // bounds is out of order; the kernel adds its own test of the warm start
    A.fast_clamp = std::isfinite(c.control_noise) ? 1 : 0;
    for (int d = 0; d < udim_of(c.model); ++d)
        if (!(c.u_min[d] <= c.u_max[d])) A.fast_clamp = 0;
    if (!fast_clamp_allowed) A.fast_clamp = 0;   // (CCV_MPPI_FAST_CLAMP=0: tests, experiments)
    const bool roll_off = (c.flags & CCV_MPPI_FLAG_ROLL_OFF) != 0;
    A.w_path = c.path_weight;
    A.w_v = c.v_weight;
    A.w_zmp = roll_off ? 0.0 : c.zmp_weight;        // fb:43-46
    A.w_rollv = roll_off ? 0.0 : c.roll_v_weight;
    A.w_back = c.back_weight;
    A.w_yaw = c.yaw_weight;
}

void fill_args(const Core* h, RolloutArgs& A, const double* x0, double dt, double yaw_ref0, uint64_t seed,
               uint64_t iter) {
    const ccv_mppi_config& c = h->cfg;
    std::memset(&A, 0, sizeof(A));
    const int nx = c.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    for (int i = 0; i < nx; ++i) A.x0[i] = x0[i];
    A.dt = dt;
    A.yaw_ref0 = yaw_ref0;
    fill_params(c, h->fast_clamp_allowed, A);
    // fb.h:212-216, fb:86-91
    const double upper_body_height = 0.8075, upper_body_width = 0.208, mass = 60.0;
    const double base2CoM = upper_body_height / 2;
    A.fb_mass = mass;
    A.fb_L = base2CoM;
    A.fb_Ixx = (mass * (upper_body_width * upper_body_width + upper_body_height * upper_body_height)) / 12 + mass * base2CoM * base2CoM;
    A.fb_gz = -9.8;  // fb.h:30
    A.inv_dt = 1.0 / dt;
    A.seed_lo = (uint32_t)seed;
    A.seed_hi = (uint32_t)(seed >> 32);
    A.iter_lo = (uint32_t)iter;
    A.iter_hi = (uint32_t)(iter >> 32);
    A.K = h->K;
    A.pitch = h->pitch;
    A.H = h->H;
    A.k_offset = c.sample_offset;
    A.steer_off = (c.flags & CCV_MPPI_FLAG_STEER_OFF) ? 1 : 0;
    A.nominal = h->d_nominal;
    A.u = h->d_u;
    A.z = h->d_z;
    A.nominal_used = h->d_nom_used;
    A.xs = h->d_xs;
    A.ys = h->d_ys;
    A.cost = h->d_cost;
    A.w = h->d_w;
    A.partial = h->d_partial;
    A.statpart = h->d_statpart;
    A.nparts = h->nblocks;
    A.fuse_update = 0;
    A.prio_rotate = h->prio_rotate;
    A.pending_vec = nullptr;
    A.nominal_w = h->d_nominal;
    A.stats_w = h->d_stats;
    A.cu_count = h->cu_count;
    A.prune = h->prune;
    A.dbg = h->d_dbg;
}

// Window coefficients relative to the current pose (px, py): |p - r_j|^2 = |p|^2 + a_j px + b_j py + c_j.  For a single
// handle's launch argument W and for every record of a batch.
void window_coeffs(const int H, const double* x_ref, const double* y_ref, const double px, const double py, double* a, double* b,
                   double* c) {
    for (int j = 0; j < H; ++j) {
        const double xl = x_ref[j] - px, yl = y_ref[j] - py;
        a[j] = -2.0 * xl;
        b[j] = -2.0 * yl;
        c[j] = xl * xl + yl * yl;
    }
}

void launch_finalize(Core& h, const UpdatePlan& p) {
    const unsigned blocks = finalize_blocks(p.args.R);
    if (p.batch && p.shift) hipLaunchKernelGGL(k_finalize_batch_shift, dim3(blocks, p.batch), dim3(kBlock), 0, h.stream, p.args, p.shift, p.K);
    else if (p.batch) hipLaunchKernelGGL(k_finalize_batch, dim3(blocks, p.batch), dim3(kBlock), 0, h.stream, p.args, p.fused ? 1 : 0);
    else hipLaunchKernelGGL(k_finalize, dim3(blocks), dim3(kBlock), 0, h.stream, p.args);
}

void launch_finalize_advance(Core& h, const UpdatePlan& p, const AdvanceArgs& V) {
    hipLaunchKernelGGL(k_finalize_advance, dim3(finalize_blocks(p.args.R) + 1), dim3(kBlock), 0, h.stream, p.args, V);
}

void launch_finalize_advance(Core& h, const UpdatePlan& p, const BatchAdvanceArgs& G, BatchParams* table, const FleetArgs* fleet,
                             const FleetPredArgs* pred) {
    const dim3 grid(finalize_blocks(p.args.R) + 1, p.batch);
    if (fleet && pred && p.shift)
        hipLaunchKernelGGL(k_finalize_advance_batch_shift_fleet_pred, grid, dim3(kBlock), 0, h.stream, p.args, G, table, *fleet, *pred);
    else if (fleet && pred) hipLaunchKernelGGL(k_finalize_advance_batch_fleet_pred, grid, dim3(kBlock), 0, h.stream, p.args, G, table, *fleet, *pred);
    else if (fleet && p.shift) hipLaunchKernelGGL(k_finalize_advance_batch_shift_fleet, grid, dim3(kBlock), 0, h.stream, p.args, G, table, *fleet);
    else if (fleet) hipLaunchKernelGGL(k_finalize_advance_batch_fleet, grid, dim3(kBlock), 0, h.stream, p.args, G, table, *fleet);
    else if (p.shift) hipLaunchKernelGGL(k_finalize_advance_batch_shift, grid, dim3(kBlock), 0, h.stream, p.args, G, p.shift);
    else if (table) hipLaunchKernelGGL(k_finalize_advance_batch_varied, grid, dim3(kBlock), 0, h.stream, p.args, G, table);
    else hipLaunchKernelGGL(k_finalize_advance_batch, grid, dim3(kBlock), 0, h.stream, p.args, G);
}

// The deferred update of a resident tick (DeferredUpdate) is launched now, as the plain update of the fused partials.
int flush_finalize(Core* h) {
    if (!h->fin_pending) return CCV_MPPI_OK;
    launch_finalize(*h, h->fin);
    h->fin_pending = false;
    HIP_TRY(h, hipGetLastError());
    return CCV_MPPI_OK;
}

// A deferred ccv_mppi_apply_partials_enqueue is normally consumed by the next fused rollout launch (pc_stage_nominal);
// anything else that reads the warm start first gets it materialised here.
int flush_division(ccv_mppi_handle* h) {
    if (!h->pending_vec) return CCV_MPPI_OK;
    hipLaunchKernelGGL(k_apply_partials, dim3(1), dim3(kBlock), 0, h->stream, h->pending_vec, h->d_nominal, h->d_stats, h->R);
    h->pending_vec = nullptr;
    HIP_TRY(h, hipGetLastError());
    return CCV_MPPI_OK;
}

int flush_pending(ccv_mppi_handle* h) {
    if (int rc = flush_finalize(h)) return rc;
    return flush_division(h);
}

// The fused kernels store the normals, not the controls; whoever needs the controls as an array (the stage-wise calls after a
// fused iteration, the unfused update) gets them re-derived into d_u first: the samplers' arithmetic, the same bits.
int materialize_controls(ccv_mppi_handle* h) {
    if (!h->controls_in_z) return CCV_MPPI_OK;
    MaterializeArgs M;
    M.z = h->d_z;
    M.nominal_used = h->d_nom_used;
    M.u = h->d_u;
    M.sigma = h->cfg.control_noise;
    for (int d = 0; d < CCV_MPPI_MAX_UDIM; ++d) {
        M.umin[d] = h->cfg.u_min[d];
        M.umax[d] = h->cfg.u_max[d];
    }
    M.K = h->K;
    M.pitch = h->pitch;
    M.R = h->R;
    M.udim = h->udim;
    M.zero_dim = (h->cfg.model == CCV_MPPI_FULL_BODY && (h->cfg.flags & CCV_MPPI_FLAG_STEER_OFF)) ? 2 : -1;
    hipLaunchKernelGGL(k_materialize_controls, dim3((h->K + kBlock - 1) / kBlock, h->R), dim3(kBlock), 0, h->stream, M);
    HIP_TRY(h, hipGetLastError());
    h->controls_in_z = false;
    return CCV_MPPI_OK;
}

// The cooperative kernels use a branch-free sin/cos that is valid for |angle| <= kFastTrigLimit.  Every heading a sample can
// reach is bounded by the start angle plus (H-1) steps at the largest control magnitude, so the decision is made here,
// once per call; anything else (huge or non-finite angles, unbounded injected controls) runs the plain
// one-sample-per-lane kernel with OCML's sincos.
// Returns kTrigUnsafe (plain kernel), kTrigSafe, or kTrigWide: diff drive, a family with a wide-turn form (has_wide: the fused
// iteration of the four-wave or one-wave kernel), every heading inside the range but a turn per step beyond pi/4 -- the
// instantiation that evaluates sin / cos of every heading in full (as the steering model's does) instead of advancing them by
// the step's turn.
// (c: the configuration whose clamp bounds apply -- h->cfg, or an instance's of a batch with per-instance parameters)
int fast_trig_safe(const Core* h, const ccv_mppi_config& c, const RolloutArgs& A, const int mode, const bool has_wide) {
    const int ud = h->udim;
    double umax[CCV_MPPI_MAX_UDIM];
    for (int d = 0; d < ud; ++d) {
        umax[d] = mode == MODE_FUSED ? std::fmax(std::fabs(c.u_min[d]), std::fabs(c.u_max[d])) : h->inj_absmax[d];
    }
    const double steps = (double)(h->H - 1) * std::fabs(A.dt);
    double bound = std::fabs(A.x0[2]) + steps * umax[1];
    if (h->cfg.model != CCV_MPPI_DIFF_DRIVE) bound += umax[2];
    if (h->cfg.model == CCV_MPPI_FULL_BODY) {
        bound = std::fmax(bound, std::fabs(A.x0[3]) + steps * umax[3]);
        bound = std::fmax(bound, std::fabs(A.x0[4]) + steps * umax[4]);
    }
    // diff drive advances (sin, cos) of the heading by the step's turn angle: needs |w| dt <= pi/4 (fast_trig.h)
    bool wide = false;
    if (h->cfg.model == CCV_MPPI_DIFF_DRIVE && !(umax[1] * std::fabs(A.dt) <= kSmallTurnLimit)) {
        if (!has_wide) return kTrigUnsafe;   // (the stage-wise and the experiment kernels have no wide form)
        wide = true;
    }
    // full body: the same for yaw, roll and pitch, and the direction angle itself is evaluated without range reduction
    if (h->cfg.model == CCV_MPPI_FULL_BODY) {
        if (!(umax[1] * std::fabs(A.dt) <= kSmallTurnLimit) || !(umax[3] * std::fabs(A.dt) <= kSmallTurnLimit) ||
            !(umax[4] * std::fabs(A.dt) <= kSmallTurnLimit) || !(umax[2] <= kSmallTurnLimit))
            return kTrigUnsafe;
        // ... and divides by dt through its reciprocal (div_uniform, mppi_device_util.h): nothing may overflow or vanish on the way
        if (!(std::fabs(A.dt) >= 1.0e-100 && std::fabs(A.dt) <= 1.0e100) || !(umax[0] <= 1.0e100) || !(umax[3] <= 1.0e100)) return kTrigUnsafe;
    }
    if (!(bound <= kFastTrigLimit)) return kTrigUnsafe;   // (also for NaN)
    return wide ? kTrigWide : kTrigSafe;
}

// the plan of a single handle's launch
RolloutPlan plan_of(const ccv_mppi_handle* h, const RolloutArgs& A, const int mode) {
    return make_plan(*h, h->cfg.model, mode, fast_trig_safe(h, h->cfg, A, mode, has_wide_form(*h, mode)), 0, BatchForm::Single, false);
}

// mode: MODE_FUSED / MODE_ROLLOUT / MODE_COST (mppi_kernels.h).  A timed fused launch carries its events on the dispatch
// itself (timing_rollout_at).
int launch_rollout(ccv_mppi_handle* h, const RolloutArgs& A_in, const Window& W, int mode) {
    RolloutArgs A = A_in;
    const RolloutPlan plan = plan_of(h, A, mode);
    const bool coop = plan.family != KernelFamily::Plain;
    // the production kernel also reduces its workgroup's share of sum w and sum w*u (no second pass over the controls);
    // the underflow-safe MIN_SHIFT mode needs the global minimum first and keeps the separate update kernels
    A.fuse_update = (coop && mode != MODE_ROLLOUT && !(h->cfg.flags & CCV_MPPI_FLAG_MIN_SHIFT)) ? 1 : 0;
    if (int rc = flush_finalize(h)) return rc;   // (the kernel reads the warm start)
    if (h->pending_vec) {
        if (coop && mode == MODE_FUSED) {   // the kernel divides while it stages u* (and writes it back)
            A.pending_vec = h->pending_vec;
            h->pending_vec = nullptr;
        } else {
            if (int rc = flush_division(h)) return rc;
        }
    }
    if (mode != MODE_ROLLOUT) h->nparts_last = A.fuse_update ? h->nblocks : 0;
    if (mode != MODE_FUSED) {   // the stage-wise kernels read the controls as an array
        if (int rc = materialize_controls(h)) return rc;
    }
    // (a timed launch of the plain kernel: events recorded around it -- the fallback must deliver kernel times too)
    LaunchAt at{h->stream, nullptr, nullptr};
    if (mode == MODE_FUSED) HIP_TRY(h, timing_rollout_at(*h, h->stream, !coop, at));
    launch_rollout(plan, at, A, W);
    if (mode == MODE_FUSED) HIP_TRY(h, timing_rollout_done(*h, h->stream, !coop));
    HIP_TRY(h, hipGetLastError());
    if (mode == MODE_FUSED) h->controls_in_z = coop;   // (the plain kernel writes u itself)
    return CCV_MPPI_OK;
}

int launch_sample(ccv_mppi_handle* h, const RolloutArgs& A) {
    if (int rc = flush_pending(h)) return rc;
    launch_sample(h->cfg.model, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return CCV_MPPI_OK;
}

// weights -> [sum w, sum w*u] (-> u* when `normalise`); vec_out may be a caller-owned device buffer.
UpdateArgs update_args(const Core* h) {
    UpdateArgs U;
    U.u = h->d_u;
    U.w = h->d_w;
    U.cost = h->d_cost;
    U.partial = h->d_partial;
    U.statpart = h->d_statpart;
    U.K = h->K;
    U.pitch = h->pitch;
    U.R = h->R;
    U.nchunks = h->nchunks;
    return U;
}

// (a batch: the first instance's slices; k_finalize_batch offsets them)
FinalizeArgs finalize_args(const Core* h, double* vec, const int nparts, const bool normalise) {
    FinalizeArgs F;
    F.partial = h->d_partial;
    F.statpart = h->d_statpart;
    F.nominal = h->d_nominal;
    F.vec = vec;
    F.stats = h->d_stats;
    F.R = h->R;
    F.nchunks = nparts;
    F.normalise = normalise ? 1 : 0;
    F.mail = nullptr;
    F.mail_seq = 0;
    return F;
}

// this update posts its result into the mailbox under the next sequence number (never 0): fetch_result() / batch_fetch() poll
void post_to_mail(Mailbox& m, FinalizeArgs& F) {
    if (++m.mail_seq == 0) m.mail_seq = 1;
    F.mail = m.d_mail;
    F.mail_seq = m.mail_seq;
    m.mail_pending = true;
}

int launch_update(ccv_mppi_handle* h, bool normalise, double* vec_out, bool exchange, bool defer) {
    if (h->fin_pending) {
        if (int rc = flush_pending(h)) return rc;
    }
    int nparts = h->nparts_last;
    if (nparts == 0) {
        // not fused (one-sample-per-lane fallback kernel or MIN_SHIFT): stream w and the controls once more
        if (int rc = materialize_controls(h)) return rc;
        if (h->cfg.flags & CCV_MPPI_FLAG_MIN_SHIFT) {
            hipLaunchKernelGGL(k_min_cost, dim3(1), dim3(1024), 0, h->stream, h->d_cost, h->K, h->d_cmin);
            hipLaunchKernelGGL(k_reweight, dim3((h->K + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->d_cost, h->d_cmin,
                               h->cfg.lambda, h->K, h->d_w);
        }
        hipLaunchKernelGGL(k_update_partials, dim3(h->nchunks, h->R + 1), dim3(kBlock), 0, h->stream, update_args(h));
        nparts = h->nchunks;
    }
    FinalizeArgs F = finalize_args(h, vec_out ? vec_out : h->d_vec, nparts, normalise);
    const bool post = h->want_mail && h->use_mail && normalise && !exchange && !defer && h->d_mail;
    h->want_mail = false;
    if (post) post_to_mail(*h, F);
    if (exchange) {
        ExchangeArgs X;
        for (int r = 0; r < kMaxRanks; ++r) X.peer[r] = h->box_peer[r];
        X.local = h->d_box;
        X.reduced = h->d_xvec;
        ++h->xchg_seq;
        X.seq = (uint32_t)(((unsigned long long)h->xchg_base + h->xchg_seq) % 0xFFFFFFFFull) + 1u;   // 1 .. 2^32-1, never 0 (the box starts zeroed)
        X.timeout_flag = h->d_xflag;
        X.world = h->xchg_world;
        X.rank = h->xchg_rank;
        X.parity = (int)(h->xchg_seq & 1);
        X.timeout_ticks = h->xchg_timeout_ticks;   // a peer that never arrives yields NaN and a flag, not a hang
        hipLaunchKernelGGL(k_finalize_exchange, dim3(finalize_blocks(h->R)), dim3(kBlock), 0, h->stream, F, X);
        HIP_TRY(h, hipGetLastError());
        h->pending_vec = h->d_xvec;   // u* = reduced[1..] / reduced[0]: deferred like ccv_mppi_apply_partials_enqueue
        return CCV_MPPI_OK;
    }
    if (defer && nparts == h->nblocks && normalise) {   // fused partials, plain update: launched with the next tick's prologue
        h->fin = UpdatePlan{F};
        h->fin_pending = true;
        return CCV_MPPI_OK;
    }
    launch_finalize(*h, UpdatePlan{F});
    HIP_TRY(h, hipGetLastError());
    return CCV_MPPI_OK;
}

// Is the launch that starts here timed (every timing_every-th is)?  Then a triple of events is reserved for it: rollout
// kernel begin, rollout kernel end, end of the launch sequence.
hipError_t timing_begin(Timing& t) {
    t.timed_now = t.timing && (t.timing_count++ % t.timing_every) == 0;
    if (!t.timed_now) return hipSuccess;
    const size_t slot = t.ev_slot = t.ev_used;
    if (t.ev.size() < slot + 3) {
        for (int i = 0; i < 3; ++i) {
            Event e;
            if (hipError_t err = e.create(/*timing=*/true)) return err;
            t.ev.push_back(std::move(e));
        }
    }
    t.ev_used += 3;
    return hipSuccess;
}

// The rollout kernel's first two events: the cooperative kernels carry them on the dispatch itself (LaunchAt), the plain kernel
// has them recorded around it -- the fallback must deliver kernel times too.
hipError_t timing_rollout_at(const Timing& t, hipStream_t stream, const bool plain, LaunchAt& at) {
    at = LaunchAt{stream, nullptr, nullptr};
    if (!t.timed_now) return hipSuccess;
    if (plain) return hipEventRecord(t.ev[t.ev_slot], stream);
    at = LaunchAt{stream, t.ev[t.ev_slot], t.ev[t.ev_slot + 1]};
    return hipSuccess;
}

hipError_t timing_rollout_done(const Timing& t, hipStream_t stream, const bool plain) {
    return t.timed_now && plain ? hipEventRecord(t.ev[t.ev_slot + 1], stream) : hipSuccess;
}

hipError_t timing_end(Timing& t, hipStream_t stream) {
    const bool timed = t.timed_now;
    t.timed_now = false;
    return timed ? hipEventRecord(t.ev[t.ev_slot + 2], stream) : hipSuccess;
}

// queue-depth throttle of the asynchronous entry points (Throttle: why)
hipError_t throttle_tick(Throttle& t, hipStream_t stream) {
    if (!t.throttle || ++t.enqueued % Throttle::kThrottleEvery != 0) return hipSuccess;
    const int ts = (int)((t.enqueued / Throttle::kThrottleEvery) % Throttle::kThrottleSlots);
    if (t.throttle_used[ts]) {
        if (hipError_t e = hipEventSynchronize(t.throttle_ev[ts])) return e;
    }
    if (hipError_t e = hipEventRecord(t.throttle_ev[ts], stream)) return e;
    t.throttle_used[ts] = true;
    return hipSuccess;
}

hipError_t timing_collect(Timing& t, hipStream_t stream) {
    if (t.ev_used == 0) return hipSuccess;
    if (hipError_t e = hipStreamSynchronize(stream)) return e;
    for (size_t s = 0; s + 3 <= t.ev_used; s += 3) {
        float a = 0.f, b = 0.f;
        if (hipError_t e = hipEventElapsedTime(&a, t.ev[s], t.ev[s + 1])) return e;
        if (hipError_t e = hipEventElapsedTime(&b, t.ev[s], t.ev[s + 2])) return e;
        t.t_roll_sum += (double)a * 1000.0;
        t.t_iter_sum += (double)b * 1000.0;
        t.t_n += 1;
        t.last_roll_us = a * 1000.f;
        t.last_iter_us = b * 1000.f;
    }
    t.ev_used = 0;
    return hipSuccess;
}

int timing_enable(Core* h, const int32_t on) {
    HIP_TRY(h, timing_collect(*h, h->stream));
    h->timing = on != 0;
    h->timing_every = on > 1 ? on : 1;   // on = n > 1: sample every n-th iteration
    h->timing_count = 0;
    return CCV_MPPI_OK;
}

int timing_read(Core* h, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters, const int32_t reset) {
    HIP_TRY(h, timing_collect(*h, h->stream));
    if (rollout_us_sum) *rollout_us_sum = h->t_roll_sum;
    if (iter_us_sum) *iter_us_sum = h->t_iter_sum;
    if (n_iters) *n_iters = h->t_n;
    if (reset) {
        h->t_roll_sum = h->t_iter_sum = 0.0;
        h->t_n = 0;
    }
    return CCV_MPPI_OK;
}

int check_iter_args(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!x0 || !x_ref || !y_ref) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!(dt == dt)) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "dt is NaN");
    return CCV_MPPI_OK;
}

// the fused iteration: sample+rollout+cost kernel, then the weighted update
// (resident: the pose and the window are taken from h->d_frame on the device; x0 then carries only the bounds on the pose
//  angles that fast_trig_safe() needs, and x_ref / y_ref are not read)
int enqueue_iteration(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref,
                      double yaw_ref0, uint64_t seed, uint64_t iter, bool normalise, double* vec_out, bool resident, bool exchange) {
    RolloutArgs A;
    Window W;
    fill_args(h, A, x0, dt, yaw_ref0, seed, iter);
    if (resident) {
        std::memset(&W, 0, sizeof(W));
        A.frame = h->d_frame;
        if (plan_of(h, A, MODE_FUSED).family == KernelFamily::Plain)
            return fail(h, CCV_MPPI_ERR_STATE, "the resident loop needs the cooperative kernels and bounded pose angles");
    } else {
        window_coeffs(h->H, x_ref, y_ref, x0[0], x0[1], W.a, W.b, W.c);
    }
    A.store_u = 1;
    A.store_xy = (h->cfg.flags & CCV_MPPI_FLAG_NO_STATE_STORE) ? 0 : 1;
    A.do_cost = 1;
    HIP_TRY(h, timing_begin(*h));
    int rc = launch_rollout(h, A, W, MODE_FUSED);
    if (rc) return rc;
    rc = launch_update(h, normalise, vec_out, exchange, /*defer=*/resident && normalise && !vec_out && !exchange && !h->timed_now);
    if (rc) return rc;
    HIP_TRY(h, timing_end(*h, h->stream));
    HIP_TRY(h, throttle_tick(*h, h->stream));
    std::memcpy(h->st_x0, A.x0, sizeof(h->st_x0));
    h->st_dt = dt;
    h->have_controls = h->have_rollout = h->have_weights = true;
    return CCV_MPPI_OK;
}

// The blocking calls' result: the update kernel has been told to post u* and the statistics into the pinned mailbox
// (FinalizeArgs::mail); poll until every packet carries this call's sequence number.  Costs the PCIe write latency after the
// kernel's last store instead of two copy-engine transfers and a stream synchronisation (C2: 72 -> ~50 us per blocking
// iteration; the reference defaults, K = 1 000, H = 15: 34 -> ~25 us).  A kernel that never posts (a fault, a lost device)
// is found by the stream query / synchronisation the poll falls back to, so the call returns an error instead of spinning.
// Then the values of the n_slots slots go to `out`: each travels as two packets {32 data bits, 32-bit sequence number}.
int read_mail(Core* h, const size_t n_slots, double* out) {
    const uint32_t seq = h->mail_seq;
    volatile unsigned long long* m = h->h_mail;
    const auto t0 = std::chrono::steady_clock::now();
    size_t next = 0;
    bool synced = false;
    for (unsigned spin = 0; next < n_slots; ++spin) {
        while (next < n_slots && (uint32_t)m[2 * next] == seq && (uint32_t)m[2 * next + 1] == seq) ++next;
        if (next == n_slots) break;
        if (synced) return fail(h, CCV_MPPI_ERR_HIP, "the update kernel finished without posting its result");
        asm volatile("" ::: "memory");
        if ((spin & 1023u) == 1023u) {
            // a long kernel (K in the millions) or a stuck one: stop burning a core after a millisecond and let the runtime wait
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (waited > 1.0e-3) {
                HIP_TRY(h, hipStreamSynchronize(h->stream));
                synced = true;   // (one more sweep: everything the kernel posted is visible now)
            }
        }
    }
    for (size_t i = 0; i < n_slots; ++i) {
        const unsigned long long hi = h->h_mail[2 * i], lo = h->h_mail[2 * i + 1];
        const unsigned long long bits = (hi & 0xFFFFFFFF00000000ull) | (lo >> 32);
        std::memcpy(&out[i], &bits, sizeof(double));
    }
    return CCV_MPPI_OK;
}

// one instance's [u* | sum w, min cost, max cost, zero-weight count] -> the caller's u* and statistics (either may be null);
// the times are those of the last timing_collect()
void unpack_result(const Timing& t, const int R, const double* v, double* u_opt_out, ccv_mppi_stats* stats) {
    const size_t n = (size_t)R;
    int nonfinite = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(v[i])) nonfinite = 1;
        if (u_opt_out) u_opt_out[i] = v[i];
    }
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    stats->sum_w = v[n + 0];
    stats->min_cost = v[n + 1];
    stats->max_cost = v[n + 2];
    stats->n_zero_weight = (int64_t)v[n + 3];
    stats->nonfinite = nonfinite;
    if (t.timing) {
        stats->device_us = t.last_iter_us;
        stats->rollout_us = t.last_roll_us;
    }
}

int fetch_result(ccv_mppi_handle* h, double* u_opt_out, ccv_mppi_stats* stats) {
    if (int rc = flush_pending(h)) return rc;
    const size_t n = (size_t)h->R;
    if (h->mail_pending) {
        h->mail_pending = false;
        if (int rc = read_mail(h, n + (stats ? 4u : 0u), h->h_pin)) return rc;
    } else {
        // one D2H of [u* | stats] through pinned memory, then a stream sync
        HIP_TRY(h, hipMemcpyAsync(h->h_pin, h->d_nominal, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_pin + n, h->d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (stats && h->timing) HIP_TRY(h, timing_collect(*h, h->stream));
    unpack_result(*h, h->R, h->h_pin, u_opt_out, stats);
    return CCV_MPPI_OK;
}

// the four-wave kernel's wave priorities: (rank + level[role] + b) mod 4 with the roles' levels per model -- noise / dynamics /
// distance / store (r4_rotate_priority, mppi_handoff.h: where the numbers are)
static int r4_prio_levels(int model) {
    auto levels = [](int noise, int dynamics, int distance, int store) { return 16 + (noise | dynamics << 2 | distance << 4 | store << 6); };
    return model == CCV_MPPI_DIFF_DRIVE ? levels(3, 2, 1, 0) : model == CCV_MPPI_STEERING_DIFF_DRIVE ? levels(2, 3, 1, 0) : levels(0, 1, 2, 3);
}

// ---- kernel-family rule ---------------------------------------------------------------------------------------------
// From the model, the workgroups (blocks of 64 samples) of one launch, the device's CUs (s.cu_count) and CCV_MPPI_KERNEL to
// k.stagewise (Plain: one sample per lane, TwoWave, ThreeWave, FourWave) and k.fused (the same, or OneWave: the one-wave kernel
// runs the fused iteration); the defaults of k.prio_rotate and k.prune follow.  `batched`: a batch handle's launch -- the same rule
// on the batch's total number of workgroups, except that the two-wave kernel has no batched form (a full-body batch beyond one
// workgroup per CU takes the one-wave kernel at once) and that CCV_MPPI_KERNEL=v1 is the only value honoured.
void select_kernels(KernelChoice& k, const Shape& s, const int64_t workgroups, const bool batched) {
    const int64_t cus = s.cu_count;
    const bool fb = s.cfg.model == CCV_MPPI_FULL_BODY;
    const char* kenv = getenv("CCV_MPPI_KERNEL");
    const bool coop = !(kenv && std::strcmp(kenv, "v1") == 0) && k.lds_window;
    const char* forced = batched || !coop ? nullptr : kenv;
    KernelFamily f = coop ? KernelFamily::TwoWave : KernelFamily::Plain;
    // diff-drive, steering: the four-wave kernel (noise / dynamics / distance / store wave, mppi_rollout_r4.h; round 2: -6 %
    // against the three-wave kernel at C2 and, unlike it, the same time in every process at C3).  Full body: its dynamics batch
    // needs 250 VGPRs, so the four-wave kernel is built for one wave per SIMD there, one workgroup per CU -- used up to that many
    // blocks of 64 samples (round 3; the reference's own K = 10 000 is 157 blocks), the two-wave kernel up to four per CU.
    // CCV_MPPI_KERNEL=pc / r3 / r4 force one where built (experiments, tests)
    if (coop && (!fb || workgroups <= cus)) f = KernelFamily::FourWave;
    if (forced && std::strcmp(forced, "r4") == 0) f = KernelFamily::FourWave;
    if (forced && std::strcmp(forced, "r3") == 0 && !fb) f = KernelFamily::ThreeWave;
    if (forced && std::strcmp(forced, "pc") == 0) f = KernelFamily::TwoWave;
    // More blocks of 64 samples than the multi-wave kernels can hold at once (4 workgroups per CU): one wave does
    // everything for its samples (mppi_rollout_solo.h) -- the SIMDs are kept busy by independent waves then, and the
    // hand-off between the waves of a workgroup is pure loss.  Measured on 256 CUs (kernel us, multi-wave vs one-wave):
    // diff drive K = 65 536: 45 vs 56; 98 304: 85 vs 80; 131 072: 106 vs 88; 524 288: 348 vs 295; steering 131 072: 135 vs
    // 117; full body 65 536: 169 vs 192; 98 304: 316 vs 291; 131 072 (C4): 374 vs 335.  CCV_MPPI_KERNEL=solo forces it.
    // (round 2, four-wave kernel against one-wave kernel, diff drive, kernel us: K = 81 920 61.0 vs 64.2; 98 304 66.0 vs 64.3;
    //  131 072 75.2 vs 71.0; 196 608 104 vs 99; steering 131 072 90.1 vs 84.0 -- the switch sits at five blocks per CU there)
    bool solo = coop && !forced && workgroups > (fb ? (batched ? 1 : 4) : 5) * cus;
    if (forced && std::strcmp(forced, "solo") == 0) solo = true;
    k.stagewise = f;
    k.fused = solo ? KernelFamily::OneWave : f;
    // wave priorities (pc_rotate_priority): measured -4 us on the three-wave kernel (C2), -3 % on the two-wave one (C4), and
    // with four levels -5 us on the four-wave kernel (43.4 -> 38.3 us at C2)
    // four-wave kernel: the roles' levels per model (r4_prio_levels)
    k.prio_rotate = f == KernelFamily::FourWave ? r4_prio_levels(s.cfg.model) : coop ? 1 : 0;
    // Exact window pruning in the distance loop (pc_prune_window).  Measured on one box, kernel us off -> on: diff drive
    // K = 65 536 49.0 -> 42.7, steering 61.7 -> 57.3 (three-wave kernels).
    // (not for windows of 16 points or fewer -- the reference default H = 15: the test costs a block about what the whole loop
    //  over such a window does; per iteration 14.6 -> 14.2 us (dd), 16.0 -> 15.3 (sd), 21.3 -> 21.0 (fb) without it)
    k.prune = (coop && s.H > 16) ? 1 : 0;
}

// ---- what ccv_mppi_create and ccv_mppi_batch_create share -------------------------------------------------------------
int check_config(const ccv_mppi_config* cfg) {
    if (cfg->abi_version != CCV_MPPI_ABI_VERSION) return CCV_MPPI_ERR_INVALID_ARG;
    if (cfg->model < CCV_MPPI_DIFF_DRIVE || cfg->model > CCV_MPPI_FULL_BODY) return CCV_MPPI_ERR_INVALID_ARG;
    if (cfg->num_samples < 1 || cfg->horizon < 3 || cfg->horizon > CCV_MPPI_MAX_HORIZON) return CCV_MPPI_ERR_INVALID_ARG;
    return CCV_MPPI_OK;
}

int check_device(const int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CCV_MPPI_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return CCV_MPPI_ERR_NO_DEVICE;
    return CCV_MPPI_OK;
}

// K, H, R of one problem; pitch: the columns of the sample axis, nblocks: the workgroups of one problem's K; the device's CUs
void set_shape(Shape& s, const ccv_mppi_config& cfg, const int pitch, const int nblocks) {
    s.cfg = cfg;
    s.udim = udim_of(cfg.model);
    s.K = cfg.num_samples;
    s.H = cfg.horizon;
    s.R = (s.H - 1) * s.udim;
    s.pitch = pitch;
    s.nchunks = (s.K + kChunk - 1) / kChunk;
    s.nblocks = nblocks;
    // The kernel-family thresholds of select_kernels() are multiples of this count.  If the query fails, the default stays: 256,
    // the CUs of the device the thresholds were measured on -- silently, since a device that cannot be queried fails create soon after.
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && prop.multiProcessorCount > 0) s.cu_count = prop.multiProcessorCount;
}

// The handle's stream, device buffers, throttle events, pinned staging and mailbox, on the current device.  On an error the
// message is in h->err and whatever exists by then goes with the handle.
int create_buffers(Core* h, const BufferCounts& n) {
    hipError_t e;
    if ((e = h->own_stream.create()) != hipSuccess) return fail(h, CCV_MPPI_ERR_HIP, "hipStreamCreate", e);
    h->stream = h->own_stream;
    const size_t P = (size_t)h->pitch;
    // The large arrays are pieces of ONE allocation, each starting on a 2 MB boundary: one mapping, one set of large page
    // fragments, seven allocator calls less per handle.
    struct Piece { void** p; size_t bytes; } pieces[] = {
        {(void**)&h->d_z, (size_t)h->R * P * sizeof(float)},
        {(void**)&h->d_xs, (size_t)h->H * P * sizeof(double)},
        {(void**)&h->d_ys, (size_t)h->H * P * sizeof(double)},
        {(void**)&h->d_u, (size_t)h->R * P * sizeof(double)},
        {(void**)&h->d_cost, P * sizeof(double)},
        {(void**)&h->d_w, P * sizeof(double)},
        {(void**)&h->d_partial, (size_t)(h->R + 1) * n.nparts_max * sizeof(double)},
    };
    constexpr size_t kPieceAlign = (size_t)2 << 20;
    size_t arena_bytes = 0;
    for (const Piece& pc : pieces) arena_bytes += (pc.bytes + kPieceAlign - 1) / kPieceAlign * kPieceAlign;
    if ((e = h->d_arena.alloc_zeroed(arena_bytes)) != hipSuccess) return fail(h, CCV_MPPI_ERR_ALLOC, "hipMalloc", e);
    {
        size_t at = 0;
        for (const Piece& pc : pieces) {
            *pc.p = h->d_arena + at;
            at += (pc.bytes + kPieceAlign - 1) / kPieceAlign * kPieceAlign;
        }
    }
    struct { DeviceArray<double>* p; size_t n; } allocs[] = {
        {&h->d_nominal, n.nominal},
        {&h->d_nom_used, (size_t)(CCV_MPPI_MAX_HORIZON + 8) * CCV_MPPI_MAX_UDIM},   // padded: read 4 at a time
        {&h->d_statpart, n.nparts_max * 3},
        {&h->d_vec, n.vec},
        {&h->d_stats, n.stats},
        {n.extra, n.n_extra},
    };
    for (auto& a : allocs)
        if ((e = a.p->alloc_zeroed(a.n)) != hipSuccess) return fail(h, CCV_MPPI_ERR_ALLOC, "hipMalloc", e);
    if (const char* tv = std::getenv("CCV_MPPI_THROTTLE")) h->throttle = std::strcmp(tv, "0") != 0;
    for (Event& te : h->throttle_ev)
        if ((e = te.create()) != hipSuccess) return fail(h, CCV_MPPI_ERR_HIP, "creating an event", e);
    h->pin_doubles = n.pin_doubles;
    if ((e = h->h_pin.alloc(h->pin_doubles, hipHostMallocDefault)) != hipSuccess) return fail(h, CCV_MPPI_ERR_ALLOC, "hipHostMalloc", e);
    if ((e = h->h_mail.alloc(n.mail_slots * 2, hipHostMallocMapped)) != hipSuccess) return fail(h, CCV_MPPI_ERR_ALLOC, "hipHostMalloc of the mailbox", e);
    // (sequence numbers start at 1: nothing in a fresh box is taken for a packet)
    std::memset(h->h_mail, 0, n.mail_slots * 2 * sizeof(unsigned long long));
    if ((e = h->h_mail.device(&h->d_mail)) != hipSuccess) return fail(h, CCV_MPPI_ERR_HIP, "hipHostGetDevicePointer(mailbox)", e);
    if (const char* mv = std::getenv("CCV_MPPI_MAILBOX")) h->use_mail = std::strcmp(mv, "0") != 0;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(h, CCV_MPPI_ERR_HIP, "hipDeviceSynchronize", e);
    return CCV_MPPI_OK;
}

// waits for the handle's work: what the handle owns goes with the delete that follows
void wait_for_streams(Core* h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream && h->own_stream != h->stream) (void)hipStreamSynchronize(h->own_stream);
}

// (the caller has launched whatever was deferred)
int set_stream(Core* h, void* hip_stream) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    for (bool& u : h->throttle_used) u = false;   // marks recorded on the old stream are complete (synchronised above)
    return CCV_MPPI_OK;
}

// The largest |u| per control dimension of rows [n / udim][udim] a caller puts into the warm start: the resident plant
// integrates u*[0], so its angle bounds must cover it (resident_bounds).  NaN sticks: no later value replaces it.
void track_absmax(const double* u, const size_t n, const int udim, double* absmax) {
    for (int d = 0; d < CCV_MPPI_MAX_UDIM; ++d) absmax[d] = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double a = std::fabs(u[i]), m = absmax[i % (size_t)udim];
        if (a != a || (m == m && a > m)) absmax[i % (size_t)udim] = a;
    }
}

}  // namespace ccv

extern "C" {

const char* ccv_mppi_version(void) { return "ccv_mppi_hip 0.1 (gfx950)"; }

int ccv_mppi_udim(int model) {
    if (model < CCV_MPPI_DIFF_DRIVE || model > CCV_MPPI_FULL_BODY) return CCV_MPPI_ERR_INVALID_ARG;
    return udim_of(model);
}

const char* ccv_mppi_last_error(const ccv_mppi_handle* h) { return h ? h->err.c_str() : "null handle"; }

int ccv_mppi_create(const ccv_mppi_config* cfg, ccv_mppi_handle** out) {
    if (!cfg || !out) return CCV_MPPI_ERR_INVALID_ARG;
    *out = nullptr;
    if (int rc = check_config(cfg)) return rc;
    // the kernels form the global sample id sample_offset + k (k < K) in int32 before it becomes the Philox counter word
    if (cfg->sample_offset < 0 || cfg->sample_offset > INT32_MAX - cfg->num_samples) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = check_device(cfg->device)) return rc;
    ccv_mppi_handle* h = new (std::nothrow) ccv_mppi_handle();
    if (!h) return CCV_MPPI_ERR_ALLOC;
    set_shape(*h, *cfg, round_up(cfg->num_samples, 64), (cfg->num_samples + kPcSamples - 1) / kPcSamples);
    // kernel selection (experiments): CCV_MPPI_WINDOW=scalar -> the plain kernel's scalar-load window variant
    const char* env = getenv("CCV_MPPI_WINDOW");
    h->lds_window = !(env && std::strcmp(env, "scalar") == 0);
    select_kernels(*h, *h, h->nblocks, /*batched=*/false);
    if (const char* pv = std::getenv("CCV_MPPI_PRIO")) {   // 0: off; 2 .. 5: the formula schedules; 16 + digits: a level table
        const int v = std::atoi(pv);
        h->prio_rotate = v == 0 ? 0 : (((v >= 2 && v <= 5) || (v >= 16 && v < 16 + 256)) && h->stagewise == KernelFamily::FourWave) ? v : h->prio_rotate;
    }
    // CCV_MPPI_PRUNE=0/1 forces the window pruning (experiments; results do not depend on it: tests/test_gpu_prune_edges.py)
    if (const char* pv = std::getenv("CCV_MPPI_PRUNE")) h->prune = std::strcmp(pv, "0") != 0;
    if (const char* pv = std::getenv("CCV_MPPI_FAST_CLAMP")) h->fast_clamp_allowed = std::strcmp(pv, "0") != 0;

    auto bail = [&](int code) {
        std::fprintf(stderr, "ccv_mppi_create: %s\n", h->err.c_str());
        ccv_mppi_destroy(h);
        return code;
    };
    const DeviceGuard guard(cfg->device);   // (the caller's current device is put back)
    hipError_t e;
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail(fail(h, CCV_MPPI_ERR_NO_DEVICE, "hipSetDevice", e));
    const size_t nparts_max = (size_t)(h->nblocks > h->nchunks ? h->nblocks : h->nchunks);
    const size_t pad = (size_t)(CCV_MPPI_MAX_HORIZON + 8) * CCV_MPPI_MAX_UDIM;   // (u* is read 4 at a time)
    const size_t R = (size_t)h->R;
    if (int rc = create_buffers(h, BufferCounts{nparts_max, /*nominal=*/pad, /*vec=*/R + 1, /*stats=*/4, &h->d_cmin, 1,
                                                /*pin_doubles=*/R + 16, /*mail_slots=*/R + 4}))
        return bail(rc);
#if defined(CCV_DIAG)
    {
        const size_t dbg_bytes = (size_t)(kDiagHeader + kDiagSlots * kDiagBlocks) * sizeof(unsigned long long);
        if ((e = h->d_dbg.alloc_zeroed(dbg_bytes / sizeof(unsigned long long))) != hipSuccess) return bail(fail(h, CCV_MPPI_ERR_ALLOC, "hipMalloc", e));
        if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(fail(h, CCV_MPPI_ERR_HIP, "hipDeviceSynchronize", e));
    }
#endif
    *out = h;
    return CCV_MPPI_OK;
}

int ccv_mppi_destroy(ccv_mppi_handle* h) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    // everything below belongs to the handle's device; the caller's current device is put back afterwards
    const DeviceGuard guard(h->cfg.device);
    (void)hipSetDevice(h->cfg.device);
    wait_for_streams(h);
    exchange_release(h);
    delete h;
    return CCV_MPPI_OK;
}

int ccv_mppi_set_stream(ccv_mppi_handle* h, void* hip_stream) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = flush_pending(h)) return rc;
    return set_stream(h, hip_stream);
}

int ccv_mppi_synchronize(ccv_mppi_handle* h) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = flush_pending(h)) return rc;   // (after this the caller may free the partials buffer)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return exchange_check(h);
}

int ccv_mppi_set_nominal(ccv_mppi_handle* h, const double* u) {
    if (!h || !u) return CCV_MPPI_ERR_INVALID_ARG;
    h->pending_vec = nullptr;   // overwritten anyway
    if (int rc = flush_pending(h)) return rc;   // (a deferred update of the resident loop must not land on top of it)
    HIP_TRY(h, hipMemcpyAsync(h->d_nominal, u, (size_t)h->R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    track_absmax(u, (size_t)h->R, h->udim, h->nom_absmax);
    return CCV_MPPI_OK;
}

int ccv_mppi_get_nominal(ccv_mppi_handle* h, double* u) {
    if (!h || !u) return CCV_MPPI_ERR_INVALID_ARG;
    if (int rc = flush_pending(h)) return rc;
    HIP_TRY(h, hipMemcpyAsync(u, h->d_nominal, (size_t)h->R * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return exchange_check(h);
}

int ccv_mppi_iterate(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref,
                     double yaw_ref0, uint64_t seed, uint64_t iter, double* u_opt_out, ccv_mppi_stats* stats) {
    int rc = check_iter_args(h, x0, dt, x_ref, y_ref);
    if (rc) return rc;
    h->want_mail = !(stats && h->timing);   // (a timed call synchronises for its events anyway)
    rc = enqueue_iteration(h, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter, true, nullptr);
    h->want_mail = false;
    if (rc) return rc;
    return fetch_result(h, u_opt_out, stats);
}

int ccv_mppi_iterate_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref,
                             double yaw_ref0, uint64_t seed, uint64_t iter) {
    int rc = check_iter_args(h, x0, dt, x_ref, y_ref);
    if (rc) return rc;
    return enqueue_iteration(h, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter, true, nullptr);
}

int ccv_mppi_partials_size(const ccv_mppi_handle* h) { return h ? h->R + 1 : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_iterate_partials_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref,
                                      const double* y_ref, double yaw_ref0, uint64_t seed, uint64_t iter,
                                      double* dev_partials) {
    int rc = check_iter_args(h, x0, dt, x_ref, y_ref);
    if (rc) return rc;
    if (!dev_partials) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "dev_partials is null");
    if (h->cfg.flags & CCV_MPPI_FLAG_MIN_SHIFT)
        return fail(h, CCV_MPPI_ERR_INVALID_ARG, "MIN_SHIFT needs a cross-device min; not supported with partials");
    return enqueue_iteration(h, x0, dt, x_ref, y_ref, yaw_ref0, seed, iter, false, dev_partials);
}

int ccv_mppi_apply_partials_enqueue(ccv_mppi_handle* h, const double* dev_partials) {
    if (!h || !dev_partials) return CCV_MPPI_ERR_INVALID_ARG;
    // deferred: the next fused rollout launch on this handle forms u* = V / S while it stages the warm start (one kernel
    // launch less per iteration); any other reader of the warm start triggers k_apply_partials first (flush_pending)
    if (int rc = flush_pending(h)) return rc;
    h->pending_vec = dev_partials;
    return CCV_MPPI_OK;
}

}  // extern "C"

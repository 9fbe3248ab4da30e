// C ABI, device-resident closed loop of a single handle (ccv_mppi_resident_*, mppi_resident.h), and what a batch's resident
// loop shares with it: the bounds on the pose angles the host never sees, and the read-out of a trace ring.
#include "capi_internal.h"

namespace ccv {

// Bounds on |yaw|, |roll|, |pitch| of a resident pose, which the host never sees: the command u*[0] is a weighted mean
// of clamped samples (or what ccv_mppi_set_nominal put there), and the plant takes an angle modulo 2 pi once it leaves
// +-kAngleRebase (rebase_angle), so the bounds stay below kAngleRebase + one step for a loop of any length.
// angle_abs: the three bounds before this tick; c: the configuration whose clamp bounds apply (an instance's own in a batch).
ResidentBounds resident_bounds(const DeviceBuffers& buf, const ccv_mppi_config& c, const double* angle_abs, const double dt,
                               const int32_t advance) {
    auto lim = [&](int d) {
        const double a = std::fmax(std::fabs(c.u_min[d]), std::fabs(c.u_max[d]));
        const double i = buf.inj_absmax[d], n = buf.nom_absmax[d];
        return (i == i && n == n) ? std::fmax(a, std::fmax(i, n)) : NAN;   // NaN sticks (fmax alone would drop it)
    };
    ResidentBounds nb{{angle_abs[0], angle_abs[1], angle_abs[2]}, 0.0};
    if (advance) {
        auto step = [&](double bound, int d) {
            const double after = bound + lim(d) * dt;
            return after <= kAngleRebase ? after : (after == after ? kAngleRebase : after);   // (beyond it the plant re-bases: |angle| <= pi)
        };
        nb.angle[0] = step(nb.angle[0], 1);
        if (c.model == CCV_MPPI_FULL_BODY) {
            nb.angle[1] = step(nb.angle[1], 3);
            nb.angle[2] = step(nb.angle[2], 4);
        }
    }
    // the prologue (k_advance) itself takes sin / cos of the OLD heading (+ the steering command)
    nb.heading = angle_abs[0] + (c.model == CCV_MPPI_DIFF_DRIVE ? 0.0 : lim(2));
    return nb;
}

// the last min(steps, cap, max_rows) rows of a trace ring of `cap` rows on the device, oldest first (after a synchronisation)
hipError_t read_trace_ring(const double* d_ring, const int64_t cap, const int64_t steps, const int32_t max_rows, double* rows,
                           int32_t* n_rows) {
    const int64_t have = steps < cap ? steps : cap;
    const int64_t n = have < max_rows ? have : max_rows;
    std::vector<double> ring((size_t)cap * 6);
    if (hipError_t e = hipMemcpy(ring.data(), d_ring, ring.size() * sizeof(double), hipMemcpyDeviceToHost)) return e;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t step = steps - n + i;
        std::memcpy(rows + i * 6, ring.data() + (step % cap) * 6, 6 * sizeof(double));
    }
    *n_rows = (int32_t)n;
    return hipSuccess;
}

}  // namespace ccv

extern "C" {

int ccv_mppi_resident_set_path(ccv_mppi_handle* h, const double* path_x, const double* path_y, int32_t n_path,
                               double resolution) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!path_x || !path_y || n_path < 1 || !(resolution > 0.0)) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "path: null, empty or resolution <= 0");
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a queued k_advance may still read the old path)
    // the new path is built beside the old one, which goes when the new one is in place; the frame and the trace at the first call
    DeviceArray<double> path, trace;
    DeviceArray<ResidentFrame> frame;
    const size_t trace_doubles = (size_t)ccv_mppi_handle::kTraceRows * 6;
    HIP_TRY(h, path.alloc((size_t)2 * n_path));
    HIP_TRY(h, hipMemcpy(path, path_x, (size_t)n_path * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(path + n_path, path_y, (size_t)n_path * sizeof(double), hipMemcpyHostToDevice));
    if (!h->d_frame) {
        HIP_TRY(h, frame.alloc_zeroed(1));
        HIP_TRY(h, trace.alloc_zeroed(trace_doubles));
        h->d_frame = std::move(frame);
        h->d_trace = std::move(trace);
    }
    h->d_path = std::move(path);
    h->n_path = n_path;
    h->path_resolution = resolution;
    return CCV_MPPI_OK;
}

int ccv_mppi_resident_set_pose(ccv_mppi_handle* h, const double* state) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!state) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "state is null");
    if (!h->d_frame) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_resident_set_path first");
    const int nx = h->cfg.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    FrameHead head{};
    for (int i = 0; i < nx; ++i) head.x0[i] = state[i];
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_frame, &head, sizeof(head), hipMemcpyHostToDevice));
    for (int i = 0; i < 3; ++i) h->res_angle_abs[i] = std::fabs(head.x0[2 + i]);
    h->res_steps = 0;
    h->have_pose = true;
    return CCV_MPPI_OK;
}

namespace {
int resident_step(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance, bool normalise, double* vec_out,
                  bool exchange = false) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    // dt is the stride of the window index (dd:160-163): as ccv_mppi_calc_ref_path, only 0 <= dt < inf is defined
    const double stride = h->cfg.v_ref * dt / h->path_resolution;
    if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "resident step: dt must be finite and not negative");
    if (!h->d_frame || !h->have_pose) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_resident_set_path and _set_pose first");
    if (!std::isfinite(stride) || stride < 0.0 || stride * h->H > 2.0e9)
        return fail(h, CCV_MPPI_ERR_INVALID_ARG, "resident step: v_ref * dt / resolution is not a usable window stride");
    const ResidentBounds nb = resident_bounds(*h, h->cfg, h->res_angle_abs, dt, advance);
    const double bounds[5] = {0.0, 0.0, nb.angle[0], nb.angle[1], nb.angle[2]};
    // everything that can refuse the step is checked BEFORE k_advance moves the pose
    {
        RolloutArgs chk;
        fill_args(h, chk, bounds, dt, 0.0, seed, iter);
        if (plan_of(h, chk, MODE_FUSED).family == KernelFamily::Plain || !(nb.heading <= kFastTrigLimit))
            return fail(h, CCV_MPPI_ERR_STATE, "the resident loop needs the cooperative kernels and bounded pose angles / commands");
    }
    const bool fuse = h->fin_pending && !h->pending_vec;   // the last tick's update is still to be launched: together with this prologue
    if (advance && !fuse) {
        if (int rc = flush_pending(h)) return rc;   // the command is u*[0]: a deferred division has to happen now
    }
    AdvanceArgs V;
    V.frame = h->d_frame;
    V.path_x = h->d_path;
    V.path_y = h->d_path + h->n_path;
    V.nominal = h->d_nominal;
    V.trace = h->d_trace;
    V.dt = dt;
    V.v_ref = h->cfg.v_ref;
    V.resolution = h->path_resolution;
    V.n_path = h->n_path;
    V.H = h->H;
    V.model = h->cfg.model;
    V.advance = advance ? 1 : 0;
    V.trace_cap = ccv_mppi_handle::kTraceRows;
    if (fuse) {
        launch_finalize_advance(*h, h->fin, V);
        h->fin_pending = false;
    } else {
        if (int rc = flush_pending(h)) return rc;
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(kAdvanceThreads), 0, h->stream, V);
    }
    HIP_TRY(h, hipGetLastError());
    h->res_steps += 1;
    for (int i = 0; i < 3; ++i) h->res_angle_abs[i] = nb.angle[i];
    return enqueue_iteration(h, bounds, dt, nullptr, nullptr, 0.0, seed, iter, normalise, vec_out, true, exchange);
}
}  // namespace

int ccv_mppi_resident_step_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance) {
    return resident_step(h, dt, seed, iter, advance, true, nullptr);
}

int ccv_mppi_resident_step_partials_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance,
                                            double* dev_partials) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!dev_partials) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "dev_partials is null");
    if (h->cfg.flags & CCV_MPPI_FLAG_MIN_SHIFT)
        return fail(h, CCV_MPPI_ERR_INVALID_ARG, "MIN_SHIFT needs a cross-device min; not supported with partials");
    return resident_step(h, dt, seed, iter, advance, false, dev_partials);
}

int ccv_mppi_resident_step_exchange_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->xchg_connected) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_exchange_create / _connect first");
    return resident_step(h, dt, seed, iter, advance, false, nullptr, true);
}

int ccv_mppi_resident_read(ccv_mppi_handle* h, double* state, int32_t* current_index, double* x_ref, double* y_ref,
                           double* yaw_ref0, int64_t* steps) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!h->d_frame || !h->have_pose) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_resident_set_path and _set_pose first");
    ResidentFrame F;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&F, h->d_frame, sizeof(F), hipMemcpyDeviceToHost));
    const int nx = h->cfg.model == CCV_MPPI_FULL_BODY ? 5 : 3;
    if (state) for (int i = 0; i < nx; ++i) state[i] = F.x0[i];
    if (current_index) *current_index = F.index;
    if (x_ref) for (int i = 0; i < h->H; ++i) x_ref[i] = F.x_ref[i];
    if (y_ref) for (int i = 0; i < h->H; ++i) y_ref[i] = F.y_ref[i];
    if (yaw_ref0) *yaw_ref0 = F.yaw_ref0;
    if (steps) *steps = F.steps;
    return CCV_MPPI_OK;
}

int ccv_mppi_resident_read_trace(ccv_mppi_handle* h, int32_t max_rows, double* rows, int32_t* n_rows) {
    if (!h) return CCV_MPPI_ERR_INVALID_ARG;
    if (!rows || !n_rows || max_rows < 0) return fail(h, CCV_MPPI_ERR_INVALID_ARG, "rows / n_rows null or max_rows < 0");
    if (!h->d_frame || !h->have_pose) return fail(h, CCV_MPPI_ERR_STATE, "ccv_mppi_resident_set_path and _set_pose first");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, read_trace_ring(h->d_trace, ccv_mppi_handle::kTraceRows, h->res_steps, max_rows, rows, n_rows));
    return CCV_MPPI_OK;
}

}  // extern "C"

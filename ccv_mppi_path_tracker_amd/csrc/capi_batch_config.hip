// C ABI, batch handles: what configures the next launch -- per-instance parameters, shifted weights, disc obstacles and their
// velocities, the fleet term and its prediction (struct ccv_mppi_batch and its parts: capi_internal.h; what a tick runs:
// capi_batch.hip; the maps of the grid term: capi_batch_maps.hip).  Every setter has one shape: validate (every check before
// anything changes), quiesce, commit the host-side state, sync_tables.  The device tables the kernels read are a function of that
// state and are written in one place.
#include "capi_internal.h"

namespace {

// whether the obstacle kernels run (BatchForm::Obst and up): static discs (ccv_mppi_batch_set_obstacles) or the fleet term
// (_resident_set_fleet); the obst_* vectors and d_obst exist then
bool obst_on(const ccv_mppi_batch* bh) { return bh->obst || bh->fleet; }

// whether the discs have velocities of their own (BatchForm::Moving without a grid): static ones
// (ccv_mppi_batch_set_obstacle_velocities) or fleet prediction
bool moving_on(const ccv_mppi_batch* bh) { return obst_on(bh) && (bh->moving || bh->fleet_pred); }

// whether the next launch reads the velocity table: the MOVING kernels, and the GRID kernels over discs -- a grid plan is a moving
// plan, and discs that have no velocities of their own get a table of zeros, over which the moving term equals the static one
// bit for bit
bool velocities_on(const ccv_mppi_batch* bh) { return moving_on(bh) || (bh->grid && obst_on(bh)); }

// the instances' present disc counts, BatchParams::n_obst as the last prologue left it (the static counts after a setter)
int read_disc_counts(ccv_mppi_batch* bh, std::vector<int32_t>& total) {
    total.resize((size_t)bh->B);
    HIP_TRY(bh, hipMemcpy2D(total.data(), sizeof(int32_t), reinterpret_cast<const char*>(bh->d_params.get()) + offsetof(BatchParams, n_obst),
                           sizeof(BatchParams), sizeof(int32_t), (size_t)bh->B, hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}
}  // namespace

namespace ccv {

// Shifted weights alone need the parameter table, B copies of the creation configuration.
BatchForm batch_form(const ccv_mppi_batch* bh) {
    return bh->grid                      ? BatchForm::Grid
           : moving_on(bh)               ? BatchForm::Moving
           : obst_on(bh)                 ? BatchForm::Obst
           : bh->varied || bh->min_shift ? BatchForm::Varied
                                         : BatchForm::Batch;
}

int quiesce(ccv_mppi_batch* bh) {
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    if (int rc = batch_flush(bh)) return rc;
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return CCV_MPPI_OK;
}

// Every derived table that the handle's present state says the next launch or prologue reads, and nothing else; the only place
// that writes them.  Every setter ends here, so the tables follow every change of the parameters, the discs, the maps, the fleet
// term and prediction.  The caller has quiesced: a queued rollout or prologue may still read the old tables.
int sync_tables(ccv_mppi_batch* bh) {
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    // the velocity table [B][32][2]: the static rows from the host copy while `moving`, every other row zero (the fleet's rows are
    // the prologue's to write, every tick, under prediction; without prediction they have to be zero)
    if (velocities_on(bh)) {
        const size_t count = (size_t)B * M * 2;
        const std::vector<double> zeros(bh->moving ? 0 : count, 0.0);
        if (!bh->d_obst_v) HIP_TRY(bh, bh->d_obst_v.alloc(count));
        HIP_TRY(bh, hipMemcpy(bh->d_obst_v, bh->moving ? bh->obst_vxy.data() : zeros.data(), count * sizeof(double), hipMemcpyHostToDevice));
    }
    // the static counts, for the fleet's prologue
    if (bh->fleet) HIP_TRY(bh, hipMemcpy(bh->d_fleet_nstatic, bh->obst_n.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
    // the parameter table [B]: the instances' configurations while `varied`, B copies of the creation configuration otherwise
    // (shifted weights alone need it)
    if (!uses_table(bh)) return CCV_MPPI_OK;
    std::vector<BatchParams> rows((size_t)B);
    for (int b = 0; b < B; ++b) {
        RolloutArgs A;
        std::memset(&A, 0, sizeof(A));
        fill_params(batch_cfg(bh, b), bh->fast_clamp_allowed, A);   // (per instance: the clamp form of its own sigma and bounds)
        BatchParams& P = rows[(size_t)b];
        std::memset(&P, 0, sizeof(P));
        P.sigma = A.sigma;
        P.lambda = A.lambda;
        P.v_ref = A.v_ref;
        for (int d = 0; d < 5; ++d) {
            P.umin[d] = A.umin[d];
            P.umax[d] = A.umax[d];
        }
        P.w_path = A.w_path;
        P.w_v = A.w_v;
        P.w_zmp = A.w_zmp;
        P.w_rollv = A.w_rollv;
        P.w_back = A.w_back;
        P.w_yaw = A.w_yaw;
        P.fast_clamp = A.fast_clamp;
        // (under the fleet term n_obst is the static count until the next resident tick's prologue writes the tick's own)
        if (obst_on(bh)) {
            P.n_obst = bh->obst_n[(size_t)b];
            P.obst = bh->d_obst + (size_t)b * M * 3;
            P.w_obs = bh->obst_w[(size_t)b];
            if (velocities_on(bh)) P.obst_v = bh->d_obst_v + (size_t)b * M * 2;
        }
        // (without discs a GRID kernel sees n_obst = 0 and reads neither table)
        if (bh->grid && bh->grid_map_of[(size_t)b] >= 0) P.grid = bh->d_grid_rows + b;
    }
    if (!bh->d_params) HIP_TRY(bh, bh->d_params.alloc((size_t)B));
    HIP_TRY(bh, hipMemcpy(bh->d_params, rows.data(), (size_t)B * sizeof(BatchParams), hipMemcpyHostToDevice));
    return CCV_MPPI_OK;
}


int fleet_restart(ccv_mppi_batch* bh, const double* xy) {
    const size_t half = (size_t)bh->B * 2;
    for (int h = 0; h < 2 && xy; ++h) HIP_TRY(bh, hipMemcpy(bh->d_fleet_xy + h * half, xy, half * sizeof(double), hipMemcpyHostToDevice));
    if (!bh->fleet_pred) return CCV_MPPI_OK;
    if (!bh->d_fleet_v) HIP_TRY(bh, bh->d_fleet_v.alloc(2 * half));
    HIP_TRY(bh, hipMemset(bh->d_fleet_v, 0, 2 * half * sizeof(double)));
    return CCV_MPPI_OK;
}

}  // namespace ccv

extern "C" {

// ---- per-instance parameters ------------------------------------------------------------------------------------------

int ccv_mppi_batch_set_params(ccv_mppi_batch* bh, const ccv_mppi_config* cfgs) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int B = bh->B;
    // the fields that fix the layout, the kernel family and the compile-time shape stay the creation configuration's; every
    // check comes before anything changes
    const ccv_mppi_config& c0 = bh->cfg;
    for (int b = 0; b < B && cfgs; ++b) {
        const ccv_mppi_config& c = cfgs[b];
        const char* field = c.abi_version != c0.abi_version       ? "abi_version"
                            : c.model != c0.model                 ? "model"
                            : c.num_samples != c0.num_samples     ? "num_samples"
                            : c.horizon != c0.horizon             ? "horizon"
                            : c.sample_offset != c0.sample_offset ? "sample_offset"
                            : c.device != c0.device               ? "device"
                            : c.flags != c0.flags                 ? "flags"
                                                                  : nullptr;
        if (field) {
            char msg[128];
            std::snprintf(msg, sizeof(msg), "set_params: instance %d: %s differs from the creation configuration", b, field);
            return fail(bh, CCV_MPPI_ERR_INVALID_ARG, msg);
        }
    }
    if (int rc = batch_flush(bh)) return rc;         // (no device switch here: DESIGN.md section 10j)
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (a queued rollout or prologue may still read the old table)
    // (null: back to the creation configuration; the shared kernels, or B copies in the table where something else needs it)
    bh->varied = cfgs != nullptr;
    if (cfgs) bh->cfgs.assign(cfgs, cfgs + B);
    else bh->cfgs.clear();
    return sync_tables(bh);
}

int ccv_mppi_batch_get_params(ccv_mppi_batch* bh, ccv_mppi_config* out) {
    if (!bh || !out) return CCV_MPPI_ERR_INVALID_ARG;
    for (int b = 0; b < bh->B; ++b) out[b] = batch_cfg(bh, b);
    return CCV_MPPI_OK;
}

// ---- shifted weights -----------------------------------------------------------------------------------------------------

int ccv_mppi_batch_set_min_shift(ccv_mppi_batch* bh, int32_t on) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const bool want = on != 0;
    if (want == bh->min_shift) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (the pending update is the old mode's)
    // The mode is no input of any table's contents, only of whether the parameter table exists.  Where it is in use already it stays
    // as it is: under the fleet term its n_obst is the last tick's count, which _resident_read_fleet shows until the next tick, and
    // a sync would put the static counts there.
    const bool had_table = uses_table(bh);
    bh->min_shift = want;
    return had_table ? CCV_MPPI_OK : sync_tables(bh);
}

int ccv_mppi_batch_get_min_shift(const ccv_mppi_batch* bh) { return bh ? (bh->min_shift ? 1 : 0) : CCV_MPPI_ERR_INVALID_ARG; }

// ---- disc obstacles -------------------------------------------------------------------------------------------------------

int ccv_mppi_batch_set_obstacles(ccv_mppi_batch* bh, const double* xyr, const int32_t* n, int32_t max_n, const double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    const bool off = !xyr || max_n == 0;
    // every check comes before anything changes
    if (!off) {
        if (max_n < 0 || max_n > M) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacles: max_n outside [0, CCV_MPPI_MAX_OBSTACLES]");
        if (!n || !weight) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
        for (int b = 0; b < B; ++b) {
            if (!valid_weight(weight[b])) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacles: a weight is negative or not finite");
            if (n[b] < 0 || n[b] > max_n) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacles: a count outside [0, max_n]");
            for (int j = 0; j < n[b]; ++j) {
                const double* o = xyr + ((size_t)b * max_n + j) * 3;
                if (!std::isfinite(o[0]) || !std::isfinite(o[1]))
                    return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacles: a centre is not finite");
                if (!(o[2] >= 0.0) || !std::isfinite(o[2]))
                    return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacles: a radius is negative or not finite");
            }
        }
    }
    if (off && !bh->obst) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    // (a new list has no velocities until it is given some; without a list there are none)
    bh->moving = false;
    bh->obst_vxy.clear();
    bh->obst = !off;
    if (!obst_on(bh)) {   // no fleet term either: back to the kernels that ran before (null / 0 / 0 in every row of the table)
        bh->obst_xyr.clear();
        bh->obst_n.clear();
        bh->obst_w.clear();
        return sync_tables(bh);
    }
    // (off under the fleet term: the static discs go; table, weights and fleet stay)
    std::vector<double> rows((size_t)B * M * 3, 0.0);
    for (int b = 0; b < B && !off; ++b)
        for (int j = 0; j < n[b]; ++j) std::memcpy(&rows[((size_t)b * M + j) * 3], xyr + ((size_t)b * max_n + j) * 3, 3 * sizeof(double));
    if (!bh->d_obst) HIP_TRY(bh, bh->d_obst.alloc(rows.size()));
    HIP_TRY(bh, hipMemcpy(bh->d_obst, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    bh->obst_xyr.swap(rows);
    if (off) bh->obst_n.assign((size_t)B, 0);
    else bh->obst_n.assign(n, n + B);
    if (!off) bh->obst_w.assign(weight, weight + B);
    return sync_tables(bh);
}

int ccv_mppi_batch_get_obstacles(ccv_mppi_batch* bh, double* xyr, int32_t* n, int32_t max_n, double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    if (max_n < 0) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_obstacles: max_n < 0");
    const bool on = obst_on(bh);   // (under the fleet term alone: no discs, the fleet's weights)
    for (int b = 0; b < B && on; ++b)
        if (xyr && bh->obst_n[(size_t)b] > max_n) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_obstacles: max_n below an instance's count");
    for (int b = 0; b < B; ++b) {
        const int nb = on ? bh->obst_n[(size_t)b] : 0;
        if (n) n[b] = nb;
        if (weight) weight[b] = on ? bh->obst_w[(size_t)b] : 0.0;
        if (xyr) {
            std::memset(xyr + (size_t)b * max_n * 3, 0, (size_t)max_n * 3 * sizeof(double));
            if (nb > 0) std::memcpy(xyr + (size_t)b * max_n * 3, &bh->obst_xyr[(size_t)b * M * 3], (size_t)nb * 3 * sizeof(double));
        }
    }
    return CCV_MPPI_OK;
}

// ---- moving discs ---------------------------------------------------------------------------------------------------------

int ccv_mppi_batch_set_obstacle_velocities(ccv_mppi_batch* bh, const double* vxy, int32_t max_n) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    // every check comes before anything changes
    if (!bh->obst) return fail(bh, CCV_MPPI_ERR_STATE, "set_obstacle_velocities: no discs are set (ccv_mppi_batch_set_obstacles)");
    if (vxy) {
        if (max_n < 0 || max_n > M)
            return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacle_velocities: max_n outside [0, CCV_MPPI_MAX_OBSTACLES]");
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < bh->obst_n[(size_t)b] && j < max_n; ++j) {
                const double* v = vxy + ((size_t)b * max_n + j) * 2;
                if (!std::isfinite(v[0]) || !std::isfinite(v[1]))
                    return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_obstacle_velocities: a velocity is not finite");
            }
    }
    if (!vxy && !bh->moving) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    // null: back to the static kernels and their bits (under fleet prediction: the static rows stand still); else rows at or past
    // an instance's count (the fleet term's rows among them) are zero
    std::vector<double> rows(vxy ? (size_t)B * M * 2 : 0, 0.0);
    for (int b = 0; b < B && vxy; ++b)
        for (int j = 0; j < bh->obst_n[(size_t)b] && j < max_n; ++j)
            std::memcpy(&rows[((size_t)b * M + j) * 2], vxy + ((size_t)b * max_n + j) * 2, 2 * sizeof(double));
    bh->obst_vxy.swap(rows);
    bh->moving = vxy != nullptr;
    return sync_tables(bh);
}

int ccv_mppi_batch_get_obstacle_velocities(ccv_mppi_batch* bh, double* vxy, int32_t max_n) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!vxy) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    if (max_n < 0 || max_n > M) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_obstacle_velocities: max_n outside [0, CCV_MPPI_MAX_OBSTACLES]");
    std::memset(vxy, 0, (size_t)B * max_n * 2 * sizeof(double));
    if (!bh->moving) return CCV_MPPI_OK;
    for (int b = 0; b < B; ++b) {
        const int nb = bh->obst_n[(size_t)b] < max_n ? bh->obst_n[(size_t)b] : max_n;
        if (nb > 0) std::memcpy(vxy + (size_t)b * max_n * 2, &bh->obst_vxy[(size_t)b * M * 2], (size_t)nb * 2 * sizeof(double));
    }
    return CCV_MPPI_OK;
}

// ---- fleet term: the robots of one resident batch keep clear of each other (mppi_fleet.h) ---------------------------------

int ccv_mppi_batch_resident_set_fleet(ccv_mppi_batch* bh, const double* radius, double range, int32_t max_neighbours, const double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    const bool off = !radius && max_neighbours == 0;
    // every check comes before anything changes
    if (!off) {
        if (!radius || !weight) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
        if (max_neighbours < 1 || max_neighbours > M)
            return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_fleet: max_neighbours outside [1, CCV_MPPI_MAX_OBSTACLES]");
        if (!(range >= 0.0) || !std::isfinite(range)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_fleet: range is negative or not finite");
        if (B > kFleetMaxBatch) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_fleet: more than 1024 instances");
        for (int b = 0; b < B; ++b) {
            if (!(radius[b] >= 0.0) || !std::isfinite(radius[b]))
                return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_fleet: a radius is negative or not finite");
            if (!valid_weight(weight[b])) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "set_fleet: a weight is negative or not finite");
        }
    }
    if (off && !bh->fleet) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (a queued rollout or prologue may still read the tables)
    if (off) {
        bh->fleet = false;
        bh->fleet_pred = false;   // (prediction is the fleet term's)
        bh->fleet_radius.clear();
        bh->fleet_range = 0.0;
        bh->fleet_maxn = 0;
        if (!bh->obst) {   // no static discs either: back to the kernels that ran before
            bh->obst_xyr.clear();
            bh->obst_n.clear();
            bh->obst_w.clear();
        }
        return sync_tables(bh);   // (the static counts again)
    }
    if (!bh->d_obst) HIP_TRY(bh, bh->d_obst.alloc((size_t)B * M * 3));
    if (!obst_on(bh)) {   // no static discs: empty lists
        bh->obst_xyr.assign((size_t)B * M * 3, 0.0);
        bh->obst_n.assign((size_t)B, 0);
        HIP_TRY(bh, hipMemcpy(bh->d_obst, bh->obst_xyr.data(), bh->obst_xyr.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!bh->d_fleet_xy) {
        DeviceArray<double> table, radii;   // (all three or none: the test above looks at the first alone)
        DeviceArray<int32_t> counts;
        HIP_TRY(bh, table.alloc((size_t)B * 4));
        HIP_TRY(bh, radii.alloc((size_t)B));
        HIP_TRY(bh, counts.alloc((size_t)B));
        bh->d_fleet_xy = std::move(table);
        bh->d_fleet_radius = std::move(radii);
        bh->d_fleet_nstatic = std::move(counts);
    }
    HIP_TRY(bh, hipMemcpy(bh->d_fleet_radius, radius, (size_t)B * sizeof(double), hipMemcpyHostToDevice));
    // the position table from the current frames (zeros before the first _set_poses, which writes it again)
    std::vector<double> xy((size_t)B * 2, 0.0);
    if (bh->have_poses)
        HIP_TRY(bh, hipMemcpy2D(xy.data(), 2 * sizeof(double), bh->d_rframe, sizeof(ResidentFrame), 2 * sizeof(double), (size_t)B,
                               hipMemcpyDeviceToHost));
    if (int rc = fleet_restart(bh, xy.data())) return rc;
    bh->obst_w.assign(weight, weight + B);
    bh->fleet_radius.assign(radius, radius + B);
    bh->fleet_range = range;
    bh->fleet_maxn = max_neighbours;
    bh->fleet = true;
    return sync_tables(bh);
}

int ccv_mppi_batch_resident_get_fleet(ccv_mppi_batch* bh, double* radius, double* range, int32_t* max_neighbours) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    for (int b = 0; b < bh->B && radius; ++b) radius[b] = bh->fleet ? bh->fleet_radius[(size_t)b] : 0.0;
    if (range) *range = bh->fleet_range;
    if (max_neighbours) *max_neighbours = bh->fleet_maxn;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_fleet(ccv_mppi_batch* bh, int32_t* n_static, int32_t* n_total, double* xyr) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->fleet) return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_fleet first");
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    if (int rc = batch_flush(bh)) return rc;   // (no device switch here: DESIGN.md section 10j)
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    std::vector<int32_t> total;
    if (int rc = read_disc_counts(bh, total)) return rc;
    if (xyr) {
        HIP_TRY(bh, hipMemcpy(xyr, bh->d_obst, (size_t)B * M * 3 * sizeof(double), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)   // (rows past the count: whatever an earlier tick left there)
            for (int j = total[(size_t)b]; j < M; ++j) std::memset(xyr + ((size_t)b * M + j) * 3, 0, 3 * sizeof(double));
    }
    for (int b = 0; b < B; ++b) {
        if (n_static) n_static[b] = bh->obst_n[(size_t)b];
        if (n_total) n_total[b] = total[(size_t)b];
    }
    return CCV_MPPI_OK;
}

// ---- fleet prediction: a neighbour's disc moves with the velocity its robot had over the last tick -------------------------

int ccv_mppi_batch_set_fleet_prediction(ccv_mppi_batch* bh, int32_t on) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->fleet) return fail(bh, CCV_MPPI_ERR_STATE, "set_fleet_prediction: the fleet term is off (ccv_mppi_batch_resident_set_fleet)");
    const bool want = on != 0;
    if (want == bh->fleet_pred) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (a queued rollout or prologue may still read the tables)
    bh->fleet_pred = want;
    if (int rc = fleet_restart(bh, nullptr)) return rc;
    // (off: the fleet's rows of the velocity table still hold what the last prologue with prediction wrote; the sync zeroes them
    // where the MOVING kernels go on reading the table for the static velocities)
    return sync_tables(bh);
}

int ccv_mppi_batch_get_fleet_prediction(const ccv_mppi_batch* bh) { return bh ? (bh->fleet_pred ? 1 : 0) : CCV_MPPI_ERR_INVALID_ARG; }

int ccv_mppi_batch_read_fleet_velocities(ccv_mppi_batch* bh, double* vxy) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!vxy) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->fleet) return fail(bh, CCV_MPPI_ERR_STATE, "ccv_mppi_batch_resident_set_fleet first");
    const int B = bh->B;
    constexpr int M = CCV_MPPI_MAX_OBSTACLES;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    std::memset(vxy, 0, (size_t)B * M * 2 * sizeof(double));
    if (!moving_on(bh)) return CCV_MPPI_OK;   // (the static kernels ran: every disc stood still)
    std::vector<int32_t> total;
    if (int rc = read_disc_counts(bh, total)) return rc;
    HIP_TRY(bh, hipMemcpy(vxy, bh->d_obst_v, (size_t)B * M * 2 * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)   // (rows past the count: whatever an earlier tick left there)
        for (int j = total[(size_t)b] < 0 ? 0 : total[(size_t)b]; j < M; ++j) std::memset(vxy + ((size_t)b * M + j) * 2, 0, 2 * sizeof(double));
    return CCV_MPPI_OK;
}

}  // extern "C"

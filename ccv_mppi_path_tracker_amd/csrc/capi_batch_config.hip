// C ABI, batch handles: what configures the next launch -- per-instance parameters, shifted weights, disc obstacles and their
// velocities, occupancy grids and the occupancy layers they can be derived from, the fleet term and its prediction (struct ccv_mppi_batch and its parts: capi_internal.h; what a
// tick runs: capi_batch.hip).  Every setter has one shape: validate (every check before anything changes), quiesce, commit the
// host-side state, sync_tables.  The device tables the kernels read are a function of that state and are written in one place.
#include "capi_internal.h"

#include <algorithm>

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

bool valid_weight(const double w) { return w >= 0.0 && std::isfinite(w); }

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
        if (!bh->d_obst_v) HIP_TRY(bh, hipMalloc(&bh->d_obst_v, count * sizeof(double)));
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
    if (!bh->d_params) HIP_TRY(bh, hipMalloc(&bh->d_params, (size_t)B * sizeof(BatchParams)));
    HIP_TRY(bh, hipMemcpy(bh->d_params, rows.data(), (size_t)B * sizeof(BatchParams), hipMemcpyHostToDevice));
    return CCV_MPPI_OK;
}

// what is wrong with a map's geometry (the checks _set_grids and _set_occupancy share, in this order), or null
const char* geometry_fault(const int32_t nx, const int32_t ny, const double resolution, const double origin_x, const double origin_y,
                           const float outside) {
    if (nx < 1 || nx > CCV_MPPI_GRID_MAX_DIM || ny < 1 || ny > CCV_MPPI_GRID_MAX_DIM || (int64_t)nx * ny > CCV_MPPI_GRID_MAX_CELLS)
        return "nx, ny outside [1, 32768] or nx * ny above 2^26";
    if (!(resolution > 0.0) || !std::isfinite(resolution) || !std::isfinite(1.0 / resolution)) return "a resolution is not positive and finite";
    if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) return "an origin is not finite";
    if (!std::isfinite(outside)) return "an outside value is not finite";
    return nullptr;
}

int refuse(ccv_mppi_batch* bh, const char* who, const char* what) { return fail(bh, CCV_MPPI_ERR_INVALID_ARG, (std::string(who) + what).c_str()); }

// map_of and weight of _set_grids / _set_occupancy
int check_map_roles(ccv_mppi_batch* bh, const char* who, const int32_t n_maps, const int32_t* map_of, const double* weight) {
    for (int b = 0; b < bh->B; ++b) {
        if (!valid_weight(weight[b])) return refuse(bh, who, "a weight is negative or not finite");
        if (map_of[b] < -1 || map_of[b] >= n_maps) return refuse(bh, who, "map_of outside [-1, n_maps)");
    }
    return CCV_MPPI_OK;
}

// the grid term off (the caller has quiesced): cells, layers and host copies go, null in every row of the table
int maps_off(ccv_mppi_batch* bh) {
    if (bh->d_grid_cells) HIP_TRY(bh, hipFree(bh->d_grid_cells));
    bh->d_grid_cells = nullptr;
    bh->drop_layers();
    bh->grid = false;
    bh->grid_maps.clear();
    bh->grid_offset.clear();
    bh->grid_map_of.clear();
    bh->grid_w.clear();
    return sync_tables(bh);
}

// A new set of maps takes the place of the old one (the caller has quiesced and filled `cells`, which the handle owns from here
// on, at `offset`): the grid rows, the host copies, the old cells freed.  geo: the maps' geometry, cells null.
int install_maps(ccv_mppi_batch* bh, std::vector<ccv_mppi_grid>& geo, float* cells, std::vector<size_t>& offset, const int32_t* map_of,
                 const double* weight) {
    const int B = bh->B;
    std::vector<GridRow> rows((size_t)B);
    std::memset(rows.data(), 0, rows.size() * sizeof(GridRow));
    for (int b = 0; b < B; ++b) {
        if (map_of[b] < 0) continue;
        const ccv_mppi_grid& g = geo[(size_t)map_of[b]];
        GridRow& r = rows[(size_t)b];
        r.origin_x = g.origin_x;
        r.origin_y = g.origin_y;
        r.inv = 1.0 / g.resolution;
        r.w = weight[b];
        r.cells = cells + offset[(size_t)map_of[b]];
        r.nx = g.nx;
        r.ny = g.ny;
        r.outside = g.outside;
    }
    hipError_t e = bh->d_grid_rows ? hipSuccess : hipMalloc(&bh->d_grid_rows, (size_t)B * sizeof(GridRow));
    if (e == hipSuccess) e = hipMemcpy(bh->d_grid_rows, rows.data(), rows.size() * sizeof(GridRow), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(cells);
        return fail(bh, CCV_MPPI_ERR_HIP, "the grid rows", e);
    }
    if (bh->d_grid_cells) (void)hipFree(bh->d_grid_cells);
    bh->d_grid_cells = cells;
    bh->grid_maps.swap(geo);
    bh->grid_offset.swap(offset);
    bh->grid_map_of.assign(map_of, map_of + B);
    bh->grid_w.assign(weight, weight + B);
    bh->grid = true;
    return CCV_MPPI_OK;
}

// the layer and the float cells that hold map m now: the second allocation after an odd number of rolls (Costmap::roll_front)
uint8_t* layer_of(const ccv_mppi_batch* bh, const int m, const bool back = false) {
    return ((bh->roll_front[(size_t)m] != 0) != back ? bh->d_occ_roll : bh->d_occ) + bh->grid_offset[(size_t)m];
}
float* cells_of(const ccv_mppi_batch* bh, const int m, const bool back = false) {
    const bool second = bh->occ && ((bh->roll_front[(size_t)m] != 0) != back);
    return (second ? bh->d_cells_roll : bh->d_grid_cells) + bh->grid_offset[(size_t)m];
}

// one inflation of the rectangle (x0, y0, w, h) of map m: the float cells from the layer, both the front ones or both the back ones
InflateArgs inflate_args(const ccv_mppi_batch* bh, const int m, const int32_t x0, const int32_t y0, const int32_t w, const int32_t h,
                         const bool back = false) {
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
    return InflateArgs{layer_of(bh, m, back), cells_of(bh, m, back), bh->d_profile + bh->profile_offset[(size_t)m], bh->occ_free[(size_t)m], g.nx,
                       g.ny, bh->occ_threshold[(size_t)m], bh->occ_radius[(size_t)m], x0, y0, w, h};
}

// the float cells of the rectangle (x0, y0, w, h) of map m from its layer, on the handle's stream
void inflate(ccv_mppi_batch* bh, const int m, const int32_t x0, const int32_t y0, const int32_t w, const int32_t h) {
    launch_inflate(inflate_args(bh, m, x0, y0, w, h), bh->stream);
}

// the instances' present disc counts, BatchParams::n_obst as the last prologue left it (the static counts after a setter)
int read_disc_counts(ccv_mppi_batch* bh, std::vector<int32_t>& total) {
    total.resize((size_t)bh->B);
    HIP_TRY(bh, hipMemcpy2D(total.data(), sizeof(int32_t), reinterpret_cast<const char*>(bh->d_params) + offsetof(BatchParams, n_obst),
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

int fleet_restart(ccv_mppi_batch* bh, const double* xy) {
    const size_t half = (size_t)bh->B * 2;
    for (int h = 0; h < 2 && xy; ++h) HIP_TRY(bh, hipMemcpy(bh->d_fleet_xy + h * half, xy, half * sizeof(double), hipMemcpyHostToDevice));
    if (!bh->fleet_pred) return CCV_MPPI_OK;
    if (!bh->d_fleet_v) HIP_TRY(bh, hipMalloc(&bh->d_fleet_v, 2 * half * sizeof(double)));
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
    if (!bh->d_obst) HIP_TRY(bh, hipMalloc(&bh->d_obst, rows.size() * sizeof(double)));
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

// ---- occupancy grids ------------------------------------------------------------------------------------------------------

int ccv_mppi_batch_set_grids(ccv_mppi_batch* bh, const ccv_mppi_grid* maps, int32_t n_maps, const int32_t* map_of, const double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "set_grids: ";
    const bool off = !maps || n_maps == 0;
    // every check comes before anything changes
    size_t total = 0;
    if (!off) {
        if (n_maps < 0) return refuse(bh, who, "n_maps < 0");
        if (!map_of || !weight) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
        for (int m = 0; m < n_maps; ++m) {
            const ccv_mppi_grid& g = maps[m];
            if (!g.cells) return refuse(bh, who, "a map has no cells");
            if (const char* f = geometry_fault(g.nx, g.ny, g.resolution, g.origin_x, g.origin_y, g.outside)) return refuse(bh, who, f);
            const size_t n = (size_t)g.nx * (size_t)g.ny;
            for (size_t i = 0; i < n; ++i)
                if (!std::isfinite(g.cells[i])) return refuse(bh, who, "a cell is not finite");
            total += n;
        }
        if (int rc = check_map_roles(bh, who, n_maps, map_of, weight)) return rc;
    }
    if (off && !bh->grid) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (a queued rollout may still read the old table, rows and cells)
    if (off) return maps_off(bh);
    // the cells of all maps are one allocation, sized by the maps: a new set is a new allocation, the old one goes when the new
    // one is filled
    float* cells = nullptr;
    HIP_TRY(bh, hipMalloc(&cells, total * sizeof(float)));
    std::vector<size_t> offset((size_t)n_maps);
    size_t at = 0;
    for (int m = 0; m < n_maps; ++m) {
        const size_t n = (size_t)maps[m].nx * (size_t)maps[m].ny;
        const hipError_t e = hipMemcpy(cells + at, maps[m].cells, n * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(cells);
            return fail(bh, CCV_MPPI_ERR_HIP, "set_grids: copying the cells", e);
        }
        offset[(size_t)m] = at;
        at += n;
    }
    std::vector<ccv_mppi_grid> geo(maps, maps + n_maps);
    for (ccv_mppi_grid& g : geo) g.cells = nullptr;
    if (int rc = install_maps(bh, geo, cells, offset, map_of, weight)) return rc;
    bh->drop_layers();   // (the cells are the caller's now)
    return sync_tables(bh);
}

int ccv_mppi_batch_get_grids(ccv_mppi_batch* bh, ccv_mppi_grid* maps, int32_t max_maps, int32_t* n_maps, int32_t* map_of, double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int n = bh->grid ? (int)bh->grid_maps.size() : 0;
    if (maps && (max_maps < 0 || max_maps < n)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_grids: max_maps below the number of maps");
    if (n_maps) *n_maps = n;
    for (int m = 0; m < n && maps; ++m) maps[m] = bh->grid_maps[(size_t)m];
    for (int b = 0; b < bh->B; ++b) {
        if (map_of) map_of[b] = bh->grid ? bh->grid_map_of[(size_t)b] : -1;
        if (weight) weight[b] = bh->grid ? bh->grid_w[(size_t)b] : 0.0;
    }
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_grid_cells(ccv_mppi_batch* bh, int32_t map, float* cells_out) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!cells_out) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->grid) return fail(bh, CCV_MPPI_ERR_STATE, "read_grid_cells: no maps are set (ccv_mppi_batch_set_grids)");
    if (map < 0 || map >= (int32_t)bh->grid_maps.size()) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "read_grid_cells: map out of range");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    // (a caller's cells: no kernel writes them, nothing to wait for; derived cells: k_inflate and the roll kernels do, in stream order)
    if (bh->occ) HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)map];
    HIP_TRY(bh, hipMemcpy(cells_out, cells_of(bh, map), (size_t)g.nx * (size_t)g.ny * sizeof(float), hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}

// ---- costmaps inflated on the device: occupancy layers behind the maps of the grid term (mppi_costmap.h) --------------------

int ccv_mppi_batch_set_occupancy(ccv_mppi_batch* bh, const ccv_mppi_occupancy* maps, const ccv_mppi_inflation* inflation, int32_t n_maps,
                                 const int32_t* map_of, const double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "set_occupancy: ";
    const bool off = !maps || n_maps == 0;
    // every check comes before anything changes
    size_t total = 0, n_profile = 0;
    if (!off) {
        if (n_maps < 0) return refuse(bh, who, "n_maps < 0");
        if (!inflation || !map_of || !weight) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
        for (int m = 0; m < n_maps; ++m) {
            const ccv_mppi_occupancy& g = maps[m];
            const ccv_mppi_inflation& f = inflation[m];
            if (!g.cells) return refuse(bh, who, "a map has no cells");
            if (const char* fault = geometry_fault(g.nx, g.ny, g.resolution, g.origin_x, g.origin_y, g.outside)) return refuse(bh, who, fault);
            if (g.threshold < 0 || g.threshold > 255) return refuse(bh, who, "a threshold outside [0, 255]");
            if (f.radius < 0 || f.radius > CCV_MPPI_INFLATE_MAX_RADIUS) return refuse(bh, who, "a radius outside [0, CCV_MPPI_INFLATE_MAX_RADIUS]");
            if (!f.profile) return refuse(bh, who, "an inflation has no profile");
            if (!std::isfinite(f.free_value)) return refuse(bh, who, "a free_value is not finite");
            const size_t np = (size_t)f.radius * (size_t)f.radius + 1;
            for (size_t i = 0; i < np; ++i)
                if (!std::isfinite(f.profile[i])) return refuse(bh, who, "a profile entry is not finite");
            total += (size_t)g.nx * (size_t)g.ny;
            n_profile += np;
        }
        if (int rc = check_map_roles(bh, who, n_maps, map_of, weight)) return rc;
    }
    if (off && !bh->grid) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (a queued rollout may still read the old table, rows and cells)
    if (off) return maps_off(bh);
    // the staging ring of the patches, at the first call (kept until destroy)
    if (!bh->h_patch) {
        HIP_TRY(bh, hipHostMalloc(&bh->h_patch, (size_t)Costmap::kPatchSlots * CCV_MPPI_OCC_PATCH_MAX_CELLS, hipHostMallocDefault));
        HIP_TRY(bh, hipHostGetDevicePointer(reinterpret_cast<void**>(&bh->d_patch), bh->h_patch, 0));
        for (hipEvent_t& e : bh->patch_ev) HIP_TRY(bh, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // cells, layers and profile tables of all maps: three allocations sized by the maps, filled before the old ones go
    float* cells = nullptr;
    uint8_t* layers = nullptr;
    float* profiles = nullptr;
    std::vector<size_t> offset((size_t)n_maps), poffset((size_t)n_maps);
    hipError_t e = hipMalloc(&cells, total * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&layers, total);
    if (e == hipSuccess) e = hipMalloc(&profiles, n_profile * sizeof(float));
    size_t at = 0, pat = 0;
    for (int m = 0; m < n_maps && e == hipSuccess; ++m) {
        const size_t n = (size_t)maps[m].nx * (size_t)maps[m].ny, np = (size_t)inflation[m].radius * (size_t)inflation[m].radius + 1;
        e = hipMemcpy(layers + at, maps[m].cells, n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(profiles + pat, inflation[m].profile, np * sizeof(float), hipMemcpyHostToDevice);
        offset[(size_t)m] = at;
        poffset[(size_t)m] = pat;
        at += n;
        pat += np;
    }
    if (e != hipSuccess) {
        free_device({cells, layers, profiles});
        return fail(bh, CCV_MPPI_ERR_HIP, "set_occupancy: allocating or copying the layers", e);
    }
    std::vector<ccv_mppi_grid> geo((size_t)n_maps);
    for (int m = 0; m < n_maps; ++m)
        geo[(size_t)m] = ccv_mppi_grid{maps[m].origin_x, maps[m].origin_y, maps[m].resolution, maps[m].outside, maps[m].nx, maps[m].ny, nullptr};
    if (int rc = install_maps(bh, geo, cells, offset, map_of, weight)) {
        free_device({layers, profiles});
        return rc;
    }
    bh->drop_layers();
    bh->d_occ = layers;
    bh->d_profile = profiles;
    bh->profile_offset.swap(poffset);
    for (int m = 0; m < n_maps; ++m) {
        bh->occ_threshold.push_back(maps[m].threshold);
        bh->occ_radius.push_back(inflation[m].radius);
        bh->occ_free.push_back(inflation[m].free_value);
        bh->roll_ox0.push_back(maps[m].origin_x);
        bh->roll_oy0.push_back(maps[m].origin_y);
    }
    // (no roll yet: every map in the first allocation, no cell moved; the second allocation went with the old layers)
    bh->roll_front.assign((size_t)n_maps, 0);
    bh->roll_cx.assign((size_t)n_maps, 0);
    bh->roll_cy.assign((size_t)n_maps, 0);
    bh->occ = true;
    // one full inflation per map; the stream is idle again before the tables point at the cells
    for (int m = 0; m < n_maps; ++m) inflate(bh, m, 0, 0, maps[m].nx, maps[m].ny);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return sync_tables(bh);
}

// Stream-ordered: the deferred resident update is not flushed (it reads no map), nothing is allocated, and the only wait is for
// the writer that last read the staging slot about to be refilled.
int ccv_mppi_batch_update_occupancy_enqueue(ccv_mppi_batch* bh, int32_t map, int32_t x0, int32_t y0, int32_t w, int32_t h, const uint8_t* patch) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "update_occupancy: ";
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "update_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (!patch) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (map < 0 || map >= (int32_t)bh->grid_maps.size()) return refuse(bh, who, "map out of range");
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)map];
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || w > g.nx - x0 || h > g.ny - y0) return refuse(bh, who, "the rectangle is not inside the map");
    if ((int64_t)w * h > CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "more than CCV_MPPI_OCC_PATCH_MAX_CELLS cells");
    const int slot = bh->patch_next;
    bh->patch_next = (slot + 1) % Costmap::kPatchSlots;
    if (bh->patch_used[slot]) HIP_TRY(bh, hipEventSynchronize(bh->patch_ev[slot]));
    const size_t at = (size_t)slot * CCV_MPPI_OCC_PATCH_MAX_CELLS;
    std::memcpy(bh->h_patch + at, patch, (size_t)w * (size_t)h);
    launch_occupancy_patch(layer_of(bh, map), g.nx, bh->d_patch + at, x0, y0, w, h, bh->stream);
    HIP_TRY(bh, hipEventRecord(bh->patch_ev[slot], bh->stream));
    bh->patch_used[slot] = true;
    // A changed cell moves the cost of cells up to R away: the patch grown by R, clipped to the map, is derived again (from layer
    // cells up to 2R from the patch).  A second launch: no workgroup of it reads a layer cell another is writing.
    const int R = bh->occ_radius[(size_t)map];
    const int32_t rx0 = x0 - R < 0 ? 0 : x0 - R, ry0 = y0 - R < 0 ? 0 : y0 - R;
    const int32_t rx1 = x0 + w + R > g.nx ? g.nx : x0 + w + R, ry1 = y0 + h + R > g.ny ? g.ny : y0 + h + R;
    inflate(bh, map, rx0, ry0, rx1 - rx0, ry1 - ry0);
    HIP_TRY(bh, hipGetLastError());
    return CCV_MPPI_OK;
}

// Stream-ordered like the patch above: after the handle's first roll (which allocates the second set of layers and cells, and
// quiesces for it like a setter) the deferred resident update is not flushed, nothing is allocated, and the only wait is for the
// launches that last read the staging slot about to be refilled.  Two launches however many maps roll.
int ccv_mppi_batch_roll_occupancy_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* map, const int32_t* dx, const int32_t* dy,
                                          const uint8_t* exposed, int32_t fill) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "roll_occupancy: ";
    // every check comes before anything changes
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "roll_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (!map || !dx || !dy) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const int n_maps = (int)bh->grid_maps.size();
    if (n < 1 || n > n_maps) return refuse(bh, who, "n outside [1, the number of maps]");
    if (!exposed && (fill < 0 || fill > 255)) return refuse(bh, who, "fill outside [0, 255]");
    constexpr int64_t kMaxOffset = (int64_t)1 << 30;
    std::vector<uint8_t> named((size_t)n_maps, 0);
    std::vector<double> ox((size_t)n), oy((size_t)n);
    size_t moved = 0, strip_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const int m = map[i];
        if (m < 0 || m >= n_maps) return refuse(bh, who, "map out of range");
        if (named[(size_t)m]) return refuse(bh, who, "a map is named twice");
        named[(size_t)m] = 1;
        const int64_t ex = dx[i], ey = dy[i];
        if (ex < -CCV_MPPI_GRID_MAX_DIM || ex > CCV_MPPI_GRID_MAX_DIM || ey < -CCV_MPPI_GRID_MAX_DIM || ey > CCV_MPPI_GRID_MAX_DIM)
            return refuse(bh, who, "|dx| or |dy| above CCV_MPPI_GRID_MAX_DIM");
        const int64_t cx = bh->roll_cx[(size_t)m] + ex, cy = bh->roll_cy[(size_t)m] + ey;
        if (cx < -kMaxOffset || cx > kMaxOffset || cy < -kMaxOffset || cy > kMaxOffset)
            return refuse(bh, who, "an accumulated offset beyond 2^30 cells");
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        // (from the accumulated cell count, one product and one sum: no drift, and a checker can restate it exactly)
        ox[(size_t)i] = bh->roll_ox0[(size_t)m] + (double)cx * g.resolution;
        oy[(size_t)i] = bh->roll_oy0[(size_t)m] + (double)cy * g.resolution;
        if (!std::isfinite(ox[(size_t)i]) || !std::isfinite(oy[(size_t)i])) return refuse(bh, who, "a rolled origin is not finite");
        if (ex == 0 && ey == 0) continue;
        ++moved;
        const size_t ax = (size_t)std::min<int64_t>(std::llabs(ex), g.nx), ay = (size_t)std::min<int64_t>(std::llabs(ey), g.ny);
        if (exposed) strip_bytes += ay * (size_t)g.nx + ((size_t)g.ny - ay) * ax;
    }
    const size_t entry_bytes = moved * sizeof(RollEntry), rect_bytes = moved * kRollMaxRects * sizeof(InflateArgs);
    if (entry_bytes + rect_bytes + strip_bytes > (size_t)CCV_MPPI_OCC_PATCH_MAX_CELLS)
        return refuse(bh, who, "tables and strips above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    // the second set of layers and cells, at the handle's first roll since the layers were set (every cell of it that is read
    // later is written first: the shift writes every layer cell, and the shift and the bands every float cell)
    if (!bh->d_occ_roll) {
        const DeviceGuard guard(bh->cfg.device);
        if (int rc = quiesce(bh)) return rc;
        const ccv_mppi_grid& last = bh->grid_maps.back();
        const size_t total = bh->grid_offset.back() + (size_t)last.nx * (size_t)last.ny;
        uint8_t* layers = nullptr;
        float* cells = nullptr;
        hipError_t e = hipMalloc(&layers, total);
        if (e == hipSuccess) e = hipMalloc(&cells, total * sizeof(float));
        if (e != hipSuccess) {
            free_device({layers, cells});
            return fail(bh, CCV_MPPI_ERR_HIP, "roll_occupancy: allocating the second set of layers and cells", e);
        }
        bh->d_occ_roll = layers;
        bh->d_cells_roll = cells;
    }
    if (moved == 0) return CCV_MPPI_OK;   // (nothing moves: no launch, no bit changes)
    const int slot = bh->patch_next;
    bh->patch_next = (slot + 1) % Costmap::kPatchSlots;
    if (bh->patch_used[slot]) HIP_TRY(bh, hipEventSynchronize(bh->patch_ev[slot]));
    // the slot: the entries, the rectangles, the strips (the kernels read all three in place)
    const size_t at = (size_t)slot * CCV_MPPI_OCC_PATCH_MAX_CELLS;
    RollEntry* entries = reinterpret_cast<RollEntry*>(bh->h_patch + at);
    InflateArgs* rects = reinterpret_cast<InflateArgs*>(bh->h_patch + at + entry_bytes);
    uint8_t* strips = bh->h_patch + at + entry_bytes + rect_bytes;
    const uint8_t* d_strips = bh->d_patch + at + entry_bytes + rect_bytes;
    size_t n_entries = 0, n_rects = 0, strip_at = 0;
    int64_t max_cells = 0;
    int32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const int m = map[i], ex = dx[i], ey = dy[i];
        if (ex == 0 && ey == 0) continue;
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        const int nx = g.nx, ny = g.ny, R = bh->occ_radius[(size_t)m];
        const size_t ax = (size_t)std::min(std::abs(ex), nx), ay = (size_t)std::min(std::abs(ey), ny);
        const size_t bytes = exposed ? ay * (size_t)nx + ((size_t)ny - ay) * ax : 0;
        if (bytes) std::memcpy(strips + strip_at, exposed + strip_at, bytes);
        entries[n_entries++] = RollEntry{layer_of(bh, m), layer_of(bh, m, true), cells_of(bh, m), cells_of(bh, m, true),
                                         exposed ? d_strips + strip_at : nullptr, ox[(size_t)i], oy[(size_t)i], nx, ny, ex, ey, fill, 0};
        strip_at += bytes;
        max_cells = std::max<int64_t>(max_cells, (int64_t)nx * ny);
        // The float cells to derive again: within R of an exposed cell (the leading band, |d| + R wide) or
        // of a cell that left the map (the trailing band, R wide), per axis; every other float cell is the shift's copy.  The
        // bands in y keep to the columns the bands in x leave: no cell is written twice.
        const int lx = ex ? std::min(std::abs(ex) + R, nx) : 0, tx = ex ? std::min(R, nx - lx) : 0;
        const int ly = ey ? std::min(std::abs(ey) + R, ny) : 0, ty = ey ? std::min(R, ny - ly) : 0;
        const int xa = ex > 0 ? tx : lx, xb = ex > 0 ? nx - lx : nx - tx;   // the columns between the bands in x
        const int32_t band[kRollMaxRects][4] = {{ex > 0 ? nx - lx : 0, 0, lx, ny},
                                                {ex > 0 ? 0 : nx - tx, 0, tx, ny},
                                                {xa, ey > 0 ? ny - ly : 0, xb - xa, ly},
                                                {xa, ey > 0 ? 0 : ny - ty, xb - xa, ty}};
        for (const auto& r : band) {
            if (r[2] < 1 || r[3] < 1) continue;
            rects[n_rects++] = inflate_args(bh, m, r[0], r[1], r[2], r[3], true);
            max_tiles = std::max(max_tiles, ((r[2] + kInflateTile - 1) / kInflateTile) * ((r[3] + kInflateTile - 1) / kInflateTile));
        }
    }
    launch_roll_shift(reinterpret_cast<const RollEntry*>(bh->d_patch + at), (int32_t)n_entries, max_cells, bh->d_grid_rows, bh->B, bh->stream);
    launch_inflate_rects(reinterpret_cast<const InflateArgs*>(bh->d_patch + at + entry_bytes), (int32_t)n_rects, max_tiles, bh->stream);
    const hipError_t launched = hipGetLastError();
    // the host's view moves at call time: the front bits, the offsets, the origins _get_grids and _get_occupancy return
    for (int i = 0; i < n; ++i) {
        const size_t m = (size_t)map[i];
        if (dx[i] == 0 && dy[i] == 0) continue;
        bh->roll_front[m] ^= 1;
        bh->roll_cx[m] += dx[i];
        bh->roll_cy[m] += dy[i];
        bh->grid_maps[m].origin_x = ox[(size_t)i];
        bh->grid_maps[m].origin_y = oy[(size_t)i];
    }
    bh->patch_used[slot] = true;
    HIP_TRY(bh, launched);
    HIP_TRY(bh, hipEventRecord(bh->patch_ev[slot], bh->stream));   // (after the second launch: both read the slot)
    return CCV_MPPI_OK;
}

// Stream-ordered like the patch and the roll above: the deferred resident update is not flushed, nothing is allocated on the
// device or pinned, and the only wait is for the launches that last read the staging slot about to be refilled.  Two launches
// however many maps are scanned; the front buffers are written in place (roll_front and the grid rows stay as they are).
int ccv_mppi_batch_scan_occupancy_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* map, const int32_t* sensor_xy, const int32_t* n_rays,
                                          const int32_t* end_xy, const uint8_t* hit, int32_t clear_value, int32_t mark_value) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "scan_occupancy: ";
    // every check comes first, then the next slot of the ring
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "scan_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (!map || !sensor_xy || !n_rays) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const int n_maps = (int)bh->grid_maps.size();
    if (n < 1 || n > n_maps) return refuse(bh, who, "n outside [1, the number of maps]");
    if (clear_value < 0 || clear_value > 255 || mark_value < 0 || mark_value > 255) return refuse(bh, who, "clear_value or mark_value outside [0, 255]");
    std::vector<uint8_t> named((size_t)n_maps, 0);
    int64_t traced = 0, total = 0;
    for (int i = 0; i < n; ++i) {
        const int m = map[i];
        if (m < 0 || m >= n_maps) return refuse(bh, who, "map out of range");
        if (named[(size_t)m]) return refuse(bh, who, "a map is named twice");
        named[(size_t)m] = 1;
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        const int32_t sx = sensor_xy[2 * (size_t)i], sy = sensor_xy[2 * (size_t)i + 1];
        if (sx < 0 || sx >= g.nx || sy < 0 || sy >= g.ny) return refuse(bh, who, "a sensor cell outside its map");
        if (n_rays[i] < 0) return refuse(bh, who, "a negative n_rays");
        if (n_rays[i] == 0) continue;
        ++traced;
        total += n_rays[i];
    }
    if (total > 0 && (!end_xy || !hit)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const size_t entry_bytes = (size_t)traced * sizeof(ScanEntry), rect_bytes = (size_t)traced * sizeof(InflateArgs);
    if ((int64_t)(entry_bytes + rect_bytes) + total * kScanRayBytes > (int64_t)CCV_MPPI_OCC_PATCH_MAX_CELLS)
        return refuse(bh, who, "tables and rays above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    // the reaches, and per entry the bounding box of the sensor cell and all end cells (every cell a ray touches lies in the box
    // of its two ends)
    std::vector<int64_t> box((size_t)n * 4);
    size_t ray = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t sx = sensor_xy[2 * (size_t)i], sy = sensor_xy[2 * (size_t)i + 1];
        int64_t* bb = &box[(size_t)i * 4];
        bb[0] = bb[2] = sx;
        bb[1] = bb[3] = sy;
        for (int r = 0; r < n_rays[i]; ++r, ++ray) {
            const int64_t ex = end_xy[2 * ray], ey = end_xy[2 * ray + 1];
            if (std::llabs(ex - sx) > CCV_MPPI_SCAN_MAX_REACH || std::llabs(ey - sy) > CCV_MPPI_SCAN_MAX_REACH)
                return refuse(bh, who, "a reach above CCV_MPPI_SCAN_MAX_REACH");
            bb[0] = std::min(bb[0], ex);
            bb[1] = std::min(bb[1], ey);
            bb[2] = std::max(bb[2], ex);
            bb[3] = std::max(bb[3], ey);
        }
    }
    if (traced == 0) return CCV_MPPI_OK;   // (nothing is traced: no launch, no bit changes)
    const int slot = bh->patch_next;
    bh->patch_next = (slot + 1) % Costmap::kPatchSlots;
    if (bh->patch_used[slot]) HIP_TRY(bh, hipEventSynchronize(bh->patch_ev[slot]));
    // the slot: the entries, the rectangles, the end cells, the hit bytes (the kernels read all four in place)
    const size_t at = (size_t)slot * CCV_MPPI_OCC_PATCH_MAX_CELLS, end_at = at + entry_bytes + rect_bytes, hit_at = end_at + (size_t)total * 2 * sizeof(int32_t);
    ScanEntry* entries = reinterpret_cast<ScanEntry*>(bh->h_patch + at);
    InflateArgs* rects = reinterpret_cast<InflateArgs*>(bh->h_patch + at + entry_bytes);
    std::memcpy(bh->h_patch + end_at, end_xy, (size_t)total * 2 * sizeof(int32_t));
    std::memcpy(bh->h_patch + hit_at, hit, (size_t)total);
    const int32_t* d_end = reinterpret_cast<const int32_t*>(bh->d_patch + end_at);
    const uint8_t* d_hit = bh->d_patch + hit_at;
    size_t k = 0;
    int32_t max_tiles = 0;
    ray = 0;
    for (int i = 0; i < n; ++i) {
        if (n_rays[i] == 0) continue;
        const int m = map[i];
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        entries[k] = ScanEntry{layer_of(bh, m), d_end + 2 * ray, d_hit + ray, g.nx, g.ny, sensor_xy[2 * (size_t)i], sensor_xy[2 * (size_t)i + 1],
                               n_rays[i], clear_value, mark_value, 0};
        ray += (size_t)n_rays[i];
        // The float cells to derive again: the box clipped to the map holds every cell the entry can
        // change; grown by R and clipped again it holds every float cell whose value can (from layer cells up to 2R from the box).
        const int64_t* bb = &box[(size_t)i * 4];
        const int R = bh->occ_radius[(size_t)m];
        const int32_t x0 = (int32_t)std::max<int64_t>(bb[0] - R, 0), y0 = (int32_t)std::max<int64_t>(bb[1] - R, 0);
        const int32_t x1 = (int32_t)std::min<int64_t>(bb[2] + R + 1, g.nx), y1 = (int32_t)std::min<int64_t>(bb[3] + R + 1, g.ny);
        rects[k++] = inflate_args(bh, m, x0, y0, x1 - x0, y1 - y0);
        max_tiles = std::max(max_tiles, ((x1 - x0 + kInflateTile - 1) / kInflateTile) * ((y1 - y0 + kInflateTile - 1) / kInflateTile));
    }
    launch_scan_trace(reinterpret_cast<const ScanEntry*>(bh->d_patch + at), (int32_t)traced, bh->stream);
    launch_inflate_rects(reinterpret_cast<const InflateArgs*>(bh->d_patch + at + entry_bytes), (int32_t)traced, max_tiles, bh->stream);
    const hipError_t launched = hipGetLastError();
    bh->patch_used[slot] = true;
    HIP_TRY(bh, launched);
    HIP_TRY(bh, hipEventRecord(bh->patch_ev[slot], bh->stream));   // (after the second launch: both read the slot)
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_get_occupancy(ccv_mppi_batch* bh, ccv_mppi_occupancy* maps, ccv_mppi_inflation* inflation, int32_t max_maps, int32_t* n_maps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int n = bh->occ ? (int)bh->grid_maps.size() : 0;
    if ((maps || inflation) && (max_maps < 0 || max_maps < n)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_occupancy: max_maps below the number of maps");
    if (n_maps) *n_maps = n;
    for (int m = 0; m < n; ++m) {
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        if (maps) maps[m] = ccv_mppi_occupancy{g.origin_x, g.origin_y, g.resolution, g.outside, g.nx, g.ny, bh->occ_threshold[(size_t)m], nullptr};
        if (inflation) inflation[m] = ccv_mppi_inflation{bh->occ_radius[(size_t)m], bh->occ_free[(size_t)m], nullptr};
    }
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_occupancy(ccv_mppi_batch* bh, int32_t map, uint8_t* out) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!out) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "read_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (map < 0 || map >= (int32_t)bh->grid_maps.size()) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "read_occupancy: map out of range");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued patch writers)
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)map];
    HIP_TRY(bh, hipMemcpy(out, layer_of(bh, map), (size_t)g.nx * (size_t)g.ny, hipMemcpyDeviceToHost));
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
    if (!bh->d_obst) HIP_TRY(bh, hipMalloc(&bh->d_obst, (size_t)B * M * 3 * sizeof(double)));
    if (!obst_on(bh)) {   // no static discs: empty lists
        bh->obst_xyr.assign((size_t)B * M * 3, 0.0);
        bh->obst_n.assign((size_t)B, 0);
        HIP_TRY(bh, hipMemcpy(bh->d_obst, bh->obst_xyr.data(), bh->obst_xyr.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!bh->d_fleet_xy) {
        HIP_TRY(bh, hipMalloc(&bh->d_fleet_xy, (size_t)B * 4 * sizeof(double)));
        HIP_TRY(bh, hipMalloc(&bh->d_fleet_radius, (size_t)B * sizeof(double)));
        HIP_TRY(bh, hipMalloc(&bh->d_fleet_nstatic, (size_t)B * sizeof(int32_t)));
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

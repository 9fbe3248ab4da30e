// C ABI, batch handles: paths planned on the device (include/ccv_mppi_plan.h; mppi_plan.h; struct ccv_mppi_batch's part Plan:
// capi_internal.h).  _set_plan has the setters' shape: validate (every check before anything changes), quiesce, allocate, commit.
// _plan_enqueue has the *_enqueue calls' (capi_batch_maps.hip): validate, take a slot of the staging ring (Staging: capi_internal.h), fill it, launch, seal it --
// no flush of the deferred resident update (it writes u*, which no plan reads), no allocation, no wait but for the launch that
// last read the slot.  The host reads no pose: an entry carries the address of the instance's resident pose.
#include "capi_internal.h"
#include "mppi_plan.h"
#include "mppi_plan_cost.h"
#include "mppi_costmap_follow.h"

namespace {

int refuse(ccv_mppi_batch* bh, const char* who, const char* what) { return fail(bh, CCV_MPPI_ERR_INVALID_ARG, (std::string(who) + what).c_str()); }

const char kNoPlan[] = "planning is not set (ccv_mppi_batch_resident_set_plan)";

static_assert(kPlanMaxField == CCV_MPPI_PLAN_MAX_FIELD && kPlanMaxPoses == CCV_MPPI_PLAN_MAX_POSES, "the header's limits");
static_assert(kPlanOk == CCV_MPPI_PLAN_OK && kPlanTruncated == CCV_MPPI_PLAN_TRUNCATED && kPlanNoStart == CCV_MPPI_PLAN_NO_START &&
                  kPlanStartBlocked == CCV_MPPI_PLAN_START_BLOCKED && kPlanGoalBlocked == CCV_MPPI_PLAN_GOAL_BLOCKED &&
                  kPlanUnreachable == CCV_MPPI_PLAN_UNREACHABLE && kPlanNotConverged == CCV_MPPI_PLAN_NOT_CONVERGED,
              "the header's status values");
static_assert(kPlanMaxPenalty == CCV_MPPI_PLAN_MAX_PENALTY, "the header's limit");

// the kernel of a plan call: k_plan_field while every multiplier is 1 -- the plan is then section 10q's in every bit, from the
// kernel that section describes -- else k_plan_field_cost
void launch_plan(const ccv_mppi_batch* bh, const PlanEntry* entries, int32_t n, float lethal, int32_t max_sweeps) {
    if (bh->plan_max_penalty == 0 || bh->plan_gain == 0.0f) launch_plan_field(entries, n, lethal, max_sweeps, bh->stream);
    else launch_plan_field_cost(entries, n, lethal, max_sweeps, bh->plan_gain, bh->plan_max_penalty, bh->stream);
}

}  // namespace

extern "C" {

int ccv_mppi_batch_resident_set_plan(ccv_mppi_batch* bh, const int32_t* capacity, int32_t keep_fields) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "resident_set_plan: ";
    // every check comes before anything changes
    if (!bh->have_paths) return fail(bh, CCV_MPPI_ERR_STATE, "resident_set_plan: ccv_mppi_batch_resident_set_paths first");
    const size_t B = (size_t)bh->B;
    size_t n_fields = 0;
    for (size_t b = 0; b < B && capacity; ++b) {
        if (capacity[b] < 0 || capacity[b] > CCV_MPPI_PLAN_MAX_POSES) return refuse(bh, who, "a capacity outside [0, CCV_MPPI_PLAN_MAX_POSES]");
        n_fields += capacity[b] > 0;
    }
    if (!capacity && !bh->plan) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;   // (a queued prologue may still read the old paths, a queued plan write them)
    // the instances as the device holds them: a plan may have changed n_path
    std::vector<BatchInstance> inst(B);
    HIP_TRY(bh, hipMemcpy(inst.data(), bh->d_inst, B * sizeof(BatchInstance), hipMemcpyDeviceToHost));
    if (!capacity) {
        bh->inst.swap(inst);
        bh->drop_plan();
        return CCV_MPPI_OK;
    }
    HIP_TRY(bh, staging_create(bh));
    // the paths laid out again with room for max(n_path, capacity) poses per instance; the present paths copied
    std::vector<int64_t> off(B);
    int64_t total = 0;
    for (size_t b = 0; b < B; ++b) {
        off[b] = total;
        total += std::max(inst[b].n_path, capacity[b]);
    }
    if (!keep_fields) n_fields = 0;
    std::vector<int32_t> rows(B * kPlanResultInts);
    for (size_t b = 0; b < B; ++b) {
        const int32_t never[kPlanResultInts] = {0, 0, -1, -1, -1, 0};
        std::memcpy(&rows[b * kPlanResultInts], never, sizeof(never));
    }
    DeviceArray<double> path;
    DeviceArray<int32_t> result;
    DeviceArray<uint16_t> fields;
    hipError_t e = path.alloc((size_t)2 * (size_t)total);
    if (e == hipSuccess) e = result.alloc(rows.size());
    if (e == hipSuccess && n_fields) e = fields.alloc(n_fields * (size_t)CCV_MPPI_PLAN_MAX_FIELD);
    if (e == hipSuccess) e = hipMemset(path, 0, (size_t)2 * (size_t)total * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(result, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    for (size_t b = 0; b < B && e == hipSuccess; ++b) {
        const size_t bytes = (size_t)inst[b].n_path * sizeof(double);
        e = hipMemcpy(path + off[b], bh->d_rpath + inst[b].path_off, bytes, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(path + total + off[b], bh->d_rpath + bh->n_total + inst[b].path_off, bytes, hipMemcpyDeviceToDevice);
    }
    for (size_t b = 0; b < B; ++b) inst[b].path_off = off[b];
    if (e == hipSuccess) e = hipMemcpy(bh->d_inst, inst.data(), B * sizeof(BatchInstance), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // (d_inst is only written after every other step went well: on a failure the old layout stands)
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "resident_set_plan: allocating or copying the paths", e);
    const bool keep = (bool)fields;
    bh->drop_plan();
    bh->d_rpath = std::move(path);
    bh->n_total = total;
    bh->inst.swap(inst);
    bh->d_plan_result = std::move(result);
    bh->d_plan_fields = std::move(fields);
    bh->plan_capacity.assign(capacity, capacity + B);
    bh->plan_field_of.assign(B, -1);
    bh->plan_dims.assign(2 * B, 0);
    int32_t at = 0;
    for (size_t b = 0; b < B && keep; ++b)
        if (capacity[b] > 0) bh->plan_field_of[b] = at++;
    bh->plan_keep = keep;
    bh->plan = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_get_plan(ccv_mppi_batch* bh, int32_t* capacity, int32_t* keep_fields) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    if (capacity) std::memcpy(capacity, bh->plan_capacity.data(), (size_t)bh->B * sizeof(int32_t));
    if (keep_fields) *keep_fields = bh->plan_keep ? 1 : 0;
    return CCV_MPPI_OK;
}

// (declared in ccv_mppi_plan_cost.h) host state only: the value every later _plan_enqueue and _plan_goals_enqueue launches with
int ccv_mppi_batch_resident_set_plan_penalty(ccv_mppi_batch* bh, float gain, int32_t max_penalty) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    if (!std::isfinite(gain) || gain < 0.0f) return refuse(bh, "resident_set_plan_penalty: ", "gain is NaN, infinite or negative");
    if (max_penalty < 0 || max_penalty > CCV_MPPI_PLAN_MAX_PENALTY) return refuse(bh, "resident_set_plan_penalty: ", "max_penalty outside [0, CCV_MPPI_PLAN_MAX_PENALTY]");
    bh->plan_gain = gain;
    bh->plan_max_penalty = max_penalty;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_get_plan_penalty(ccv_mppi_batch* bh, float* gain, int32_t* max_penalty) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    if (gain) *gain = bh->plan_gain;
    if (max_penalty) *max_penalty = bh->plan_max_penalty;
    return CCV_MPPI_OK;
}

}  // extern "C"

namespace {

// _plan_enqueue (goal_xy: cells) and _plan_goals_enqueue (world_xy: world points; goal_xy null; while the maps follow only).  One launch however many
// instances plan (k_plan_field), and while the maps follow one small launch ahead of it that completes the entries from the maps'
// frames (mppi_costmap_follow.h).  The poses are the device's: nothing here reads one.
int plan_enqueue(ccv_mppi_batch* bh, const char* who, int32_t n, const int32_t* instance, const int32_t* goal_xy, const double* world_xy, float lethal,
                 int32_t max_sweeps) {
    // every check comes first, then the next slot of the ring
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    if (!bh->have_paths || !bh->have_poses) return fail(bh, CCV_MPPI_ERR_STATE, (std::string(who) + "ccv_mppi_batch_resident_set_poses first").c_str());
    // (a world goal is for the caller who cannot know the frame; one who can has batch.goal_cells and _plan_enqueue)
    if (world_xy && !bh->follow) return fail(bh, CCV_MPPI_ERR_STATE, (std::string(who) + "following is not set (ccv_mppi_batch_resident_set_follow)").c_str());
    if (!instance || (!goal_xy && !world_xy)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (n < 1 || n > bh->B) return refuse(bh, who, "n outside [1, B]");
    const bool followed = bh->follow;
    if (lethal != lethal) return refuse(bh, who, "lethal is NaN");
    if (max_sweeps < 1 || max_sweeps > CCV_MPPI_PLAN_MAX_FIELD) return refuse(bh, who, "max_sweeps outside [1, CCV_MPPI_PLAN_MAX_FIELD]");
    if ((size_t)n * (followed ? sizeof(PlanFollowEntry) : sizeof(PlanEntry)) > (size_t)CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "entries above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    std::vector<uint8_t> named((size_t)bh->B, 0);
    for (int i = 0; i < n; ++i) {
        const int b = instance[i];
        if (b < 0 || b >= bh->B) return refuse(bh, who, "instance out of range");
        if (named[(size_t)b]) return refuse(bh, who, "an instance is named twice");
        named[(size_t)b] = 1;
        const int m = bh->grid ? bh->grid_map_of[(size_t)b] : -1;
        if (m < 0) return refuse(bh, who, "an instance without a map");
        if (bh->plan_capacity[(size_t)b] < 1) return refuse(bh, who, "an instance with capacity 0");
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        if (((int64_t)g.nx + 2) * ((int64_t)g.ny + 2) > CCV_MPPI_PLAN_MAX_FIELD) return refuse(bh, who, "a map above CCV_MPPI_PLAN_MAX_FIELD: (nx + 2)(ny + 2)");
        if (world_xy) {
            if (!std::isfinite(world_xy[2 * (size_t)i]) || !std::isfinite(world_xy[2 * (size_t)i + 1])) return refuse(bh, who, "a goal is not finite");
        } else {
            const int32_t gx = goal_xy[2 * (size_t)i], gy = goal_xy[2 * (size_t)i + 1];
            if (gx < 0 || gx >= g.nx || gy < 0 || gy >= g.ny) return refuse(bh, who, "a goal outside the map");
        }
        if (std::memcmp(&g.resolution, &bh->inst[(size_t)b].resolution, sizeof(double)) != 0)
            return refuse(bh, who, "a path's resolution differs from its map's");
    }
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    PlanEntry* entries = reinterpret_cast<PlanEntry*>(slot.host);
    PlanFollowEntry* wide = reinterpret_cast<PlanFollowEntry*>(slot.host);
    for (int i = 0; i < n; ++i) {
        const size_t b = (size_t)instance[i];
        const int m = bh->grid_map_of[b];
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        PlanEntry& e = followed ? wide[i].entry : entries[i];
        e.cells = cells_of(bh, m);
        e.pose = bh->d_rframe[b].x0;   // (an address: the host reads no pose)
        e.path_x = bh->d_rpath + bh->inst[b].path_off;
        e.path_y = e.path_x + bh->n_total;
        e.inst = bh->d_inst + b;
        e.result = bh->d_plan_result + b * kPlanResultInts;
        e.field = bh->plan_field_of[b] >= 0 ? bh->d_plan_fields + (size_t)bh->plan_field_of[b] * CCV_MPPI_PLAN_MAX_FIELD : nullptr;
        e.origin_x = g.origin_x;
        e.origin_y = g.origin_y;
        e.inv = 1.0 / g.resolution;
        e.resolution = g.resolution;
        e.nx = g.nx;
        e.ny = g.ny;
        // (while the maps follow, the origin and a world goal's cell are the device's to form)
        e.goal_x = goal_xy ? goal_xy[2 * (size_t)i] : 0;
        e.goal_y = goal_xy ? goal_xy[2 * (size_t)i + 1] : 0;
        if (followed) {
            wide[i].frame = bh->d_follow_frames + 2 * (size_t)m + bh->follow_slot[(size_t)m];
            wide[i].goal_wx = world_xy ? world_xy[2 * (size_t)i] : 0.0;
            wide[i].goal_wy = world_xy ? world_xy[2 * (size_t)i + 1] : 0.0;
            wide[i].world_goal = world_xy ? 1 : 0;
            wide[i].pad = 0;
        }
        e.capacity = bh->plan_capacity[b];
        e.pad[0] = e.pad[1] = e.pad[2] = 0;
        bh->plan_dims[2 * b] = g.nx;
        bh->plan_dims[2 * b + 1] = g.ny;
    }
    if (followed) {
        launch_follow_resolve_plan(reinterpret_cast<const PlanFollowEntry*>(slot.device), bh->d_follow_plan, n, bh->stream);
        launch_plan(bh, bh->d_follow_plan, n, lethal, max_sweeps);
    } else {
        launch_plan(bh, reinterpret_cast<const PlanEntry*>(slot.device), n, lethal, max_sweeps);
    }
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));
    return CCV_MPPI_OK;
}

}  // namespace

extern "C" {

int ccv_mppi_batch_resident_plan_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* instance, const int32_t* goal_xy, float lethal,
                                         int32_t max_sweeps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    return plan_enqueue(bh, "resident_plan: ", n, instance, goal_xy, nullptr, lethal, max_sweeps);
}

// (declared in ccv_mppi_follow.h: the call a caller needs who cannot know the frame)
int ccv_mppi_batch_resident_plan_goals_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* instance, const double* goal_xy, float lethal,
                                               int32_t max_sweeps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    return plan_enqueue(bh, "resident_plan_goals: ", n, instance, nullptr, goal_xy, lethal, max_sweeps);
}

int ccv_mppi_batch_resident_read_plan(ccv_mppi_batch* bh, int32_t* status, int32_t* poses, int32_t* start_cell, int32_t* start_dist, int32_t* sweeps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued plans)
    const size_t B = (size_t)bh->B;
    std::vector<int32_t> rows(B * kPlanResultInts);
    HIP_TRY(bh, hipMemcpy(rows.data(), bh->d_plan_result, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        const int32_t* r = &rows[b * kPlanResultInts];
        if (status) status[b] = r[0];
        if (poses) poses[b] = r[1];
        if (start_cell) std::memcpy(start_cell + 2 * b, r + 2, 2 * sizeof(int32_t));
        if (start_dist) start_dist[b] = r[4];
        if (sweeps) sweeps[b] = r[5];
    }
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_plan_field(ccv_mppi_batch* bh, int32_t instance, uint16_t* out) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!out) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->plan) return fail(bh, CCV_MPPI_ERR_STATE, kNoPlan);
    if (instance < 0 || instance >= bh->B) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "instance out of range");
    const int32_t slot = bh->plan_field_of[(size_t)instance];
    if (!bh->plan_keep || slot < 0) return fail(bh, CCV_MPPI_ERR_STATE, "resident_read_plan_field: no field is kept for the instance (keep_fields, capacity)");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued plans)
    int32_t status = 0;
    HIP_TRY(bh, hipMemcpy(&status, bh->d_plan_result + (size_t)instance * kPlanResultInts, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (status != kPlanOk && status != kPlanTruncated && status != kPlanUnreachable)
        return fail(bh, CCV_MPPI_ERR_STATE, "resident_read_plan_field: the instance's last plan left no field (its status is not 1, 2 or 6)");
    const size_t cells = (size_t)bh->plan_dims[2 * (size_t)instance] * (size_t)bh->plan_dims[2 * (size_t)instance + 1];
    HIP_TRY(bh, hipMemcpy(out, bh->d_plan_fields + (size_t)slot * CCV_MPPI_PLAN_MAX_FIELD, cells * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_path(ccv_mppi_batch* bh, int32_t instance, int32_t max_poses, double* x, double* y, int32_t* n_path) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!n_path || max_poses < 0 || (max_poses > 0 && (!x || !y))) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "n_path null, max_poses < 0 or x / y null");
    if (instance < 0 || instance >= bh->B) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "instance out of range");
    if (!bh->have_paths) return fail(bh, CCV_MPPI_ERR_STATE, "resident_read_path: ccv_mppi_batch_resident_set_paths first");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued plans)
    BatchInstance row;
    HIP_TRY(bh, hipMemcpy(&row, bh->d_inst + instance, sizeof(BatchInstance), hipMemcpyDeviceToHost));
    *n_path = row.n_path;
    const size_t bytes = (size_t)std::min(row.n_path, max_poses) * sizeof(double);
    if (bytes) {
        HIP_TRY(bh, hipMemcpy(x, bh->d_rpath + row.path_off, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(bh, hipMemcpy(y, bh->d_rpath + bh->n_total + row.path_off, bytes, hipMemcpyDeviceToHost));
    }
    return CCV_MPPI_OK;
}

}  // extern "C"

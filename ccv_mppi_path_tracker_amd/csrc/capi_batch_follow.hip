// C ABI, batch handles: costmaps that follow their robots (include/ccv_mppi_follow.h; mppi_costmap_follow.h; struct
// ccv_mppi_batch's part Follow: capi_internal.h).  _set_follow has the setters' shape: validate, quiesce, allocate, commit.
// _follow_enqueue has the *_enqueue calls' (capi_batch_maps.hip): validate, take a slot of the staging ring, fill it, launch, seal
// it -- no flush of the deferred resident update (it writes u*, which nothing here reads), no allocation, no wait but for the
// launches that last read the slot.  The host reads no pose and no frame: an entry carries their addresses.  What the sensor
// and the planner do while following is set stands with them (capi_batch_maps.hip, capi_batch_plan.hip).
#include "capi_internal.h"
#include "mppi_costmap_follow.h"

namespace {

int refuse(ccv_mppi_batch* bh, const char* who, const char* what) { return fail(bh, CCV_MPPI_ERR_INVALID_ARG, (std::string(who) + what).c_str()); }

const char kNoFollow[] = "following is not set (ccv_mppi_batch_resident_set_follow)";

static_assert(kFollowMoved == CCV_MPPI_FOLLOW_MOVED && kFollowHeld == CCV_MPPI_FOLLOW_HELD && kFollowNoPose == CCV_MPPI_FOLLOW_NO_POSE &&
                  kFollowLimit == CCV_MPPI_FOLLOW_LIMIT,
              "the header's status values");

}  // namespace

namespace ccv {

int follow_refresh(ccv_mppi_batch* bh) {
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued follows)
    const size_t n_maps = bh->grid_maps.size();
    std::vector<FollowFrame> frames(2 * n_maps);
    HIP_TRY(bh, hipMemcpy(frames.data(), bh->d_follow_frames, frames.size() * sizeof(FollowFrame), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n_maps; ++m) {
        const FollowFrame& f = frames[2 * m + bh->follow_slot[m]];
        bh->layers[m].cx = f.cx;
        bh->layers[m].cy = f.cy;
        bh->grid_maps[m].origin_x = f.origin_x;
        bh->grid_maps[m].origin_y = f.origin_y;
    }
    return CCV_MPPI_OK;
}

}  // namespace ccv

extern "C" {

int ccv_mppi_batch_resident_set_follow(ccv_mppi_batch* bh, int32_t on) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!on) {
        if (!bh->follow) return CCV_MPPI_OK;
        const DeviceGuard guard(bh->cfg.device);
        if (int rc = quiesce(bh)) return rc;
        if (int rc = follow_refresh(bh)) return rc;   // (the host's layers speak for the maps again)
        bh->drop_follow();
        return CCV_MPPI_OK;
    }
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "resident_set_follow: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (bh->follow) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    if (int rc = ensure_roll_buffers(bh)) return rc;
    const size_t n_maps = bh->grid_maps.size(), B = (size_t)bh->B;
    std::vector<FollowFrame> frames(2 * n_maps);
    for (size_t m = 0; m < n_maps; ++m)
        frames[2 * m] = frames[2 * m + 1] = FollowFrame{bh->layers[m].cx, bh->layers[m].cy, bh->grid_maps[m].origin_x, bh->grid_maps[m].origin_y};
    DeviceArray<FollowFrame> d_frames;
    DeviceArray<int32_t> d_result;
    DeviceArray<InflateArgs> d_rects;
    DeviceArray<SenseEntry> d_sense;
    DeviceArray<PlanEntry> d_plan;
    hipError_t e = d_frames.alloc(frames.size());
    if (e == hipSuccess) e = d_result.alloc_zeroed(n_maps * kFollowResultInts);   // (status 0: never followed)
    if (e == hipSuccess) e = d_rects.alloc_zeroed(n_maps * kFollowRects);
    if (e == hipSuccess) e = d_sense.alloc_zeroed(B);
    if (e == hipSuccess) e = d_plan.alloc_zeroed(B);
    if (e == hipSuccess) e = hipMemcpy(d_frames, frames.data(), frames.size() * sizeof(FollowFrame), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "resident_set_follow: allocating the frame table", e);
    bh->d_follow_frames = std::move(d_frames);
    bh->d_follow_result = std::move(d_result);
    bh->d_follow_rects = std::move(d_rects);
    bh->d_follow_sense = std::move(d_sense);
    bh->d_follow_plan = std::move(d_plan);
    bh->follow_slot.assign(n_maps, 0);
    bh->follow = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_get_follow(ccv_mppi_batch* bh, int32_t* on) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!on) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    *on = bh->follow ? 1 : 0;
    return CCV_MPPI_OK;
}

// Two launches however many robots follow: k_follow_shift and the inflation of the bands it wrote.
int ccv_mppi_batch_resident_follow_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* instance, int32_t margin, int32_t max_step, int32_t fill) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "resident_follow: ";
    // every check comes first, then the next slot of the ring
    if (!bh->follow) return fail(bh, CCV_MPPI_ERR_STATE, kNoFollow);
    if (!bh->have_paths || !bh->have_poses) return fail(bh, CCV_MPPI_ERR_STATE, "resident_follow: ccv_mppi_batch_resident_set_paths and _set_poses first");
    if (!instance) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (n < 1 || n > bh->B) return refuse(bh, who, "n outside [1, B]");
    if (margin < 0 || margin > CCV_MPPI_GRID_MAX_DIM) return refuse(bh, who, "margin outside [0, CCV_MPPI_GRID_MAX_DIM]");
    if (max_step < 1 || max_step > CCV_MPPI_GRID_MAX_DIM) return refuse(bh, who, "max_step outside [1, CCV_MPPI_GRID_MAX_DIM]");
    if (fill < 0 || fill > 255) return refuse(bh, who, "fill outside [0, 255]");
    if ((size_t)n * sizeof(FollowEntry) > (size_t)CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "entries above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    std::vector<uint8_t> named_b((size_t)bh->B, 0), named_m(bh->grid_maps.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int b = instance[i];
        if (b < 0 || b >= bh->B) return refuse(bh, who, "instance out of range");
        if (named_b[(size_t)b]) return refuse(bh, who, "an instance is named twice");
        named_b[(size_t)b] = 1;
        const int m = bh->grid_map_of[(size_t)b];
        if (m < 0) return refuse(bh, who, "an instance without a map");
        if (named_m[(size_t)m]) return refuse(bh, who, "two named instances on one map");
        named_m[(size_t)m] = 1;
    }
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    FollowEntry* entries = reinterpret_cast<FollowEntry*>(slot.host);
    int64_t max_cells = 0;
    int32_t max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        const size_t b = (size_t)instance[i];
        const int m = bh->grid_map_of[b];
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        Costmap::Layer& l = bh->layers[(size_t)m];
        uint8_t& at = bh->follow_slot[(size_t)m];
        FollowEntry& e = entries[i];
        e.layer_src = layer_of(bh, m, false);
        e.layer_dst = layer_of(bh, m, true);
        e.cells_src = cells_of(bh, m, false);
        e.cells_dst = cells_of(bh, m, true);
        e.rect = InflateArgs{e.layer_dst, e.cells_dst, bh->d_profile + l.profile_offset, l.free_value, g.nx, g.ny, l.threshold, l.radius, 0, 0, 0, 0};
        e.pose = bh->d_rframe[b].x0;   // (an address: the host reads no pose)
        e.frame_src = bh->d_follow_frames + 2 * (size_t)m + at;
        e.frame_dst = bh->d_follow_frames + 2 * (size_t)m + (at ^ 1);
        e.result = bh->d_follow_result + (size_t)m * kFollowResultInts;
        e.ox0 = l.ox0;
        e.oy0 = l.oy0;
        e.resolution = g.resolution;
        e.inv = 1.0 / g.resolution;
        e.nx = g.nx;
        e.ny = g.ny;
        e.margin = margin;
        e.max_step = max_step;
        e.fill = fill;
        e.pad[0] = e.pad[1] = e.pad[2] = 0;
        max_cells = std::max<int64_t>(max_cells, (int64_t)g.nx * g.ny);
        // the largest bands the device can form: min(max_step + R, n) cells of one axis over the whole of the other
        const int32_t bx = (int32_t)std::min<int64_t>((int64_t)max_step + l.radius, g.nx), by = (int32_t)std::min<int64_t>((int64_t)max_step + l.radius, g.ny);
        max_tiles = std::max(max_tiles, std::max(inflate_tiles(bx, g.ny), inflate_tiles(g.nx, by)));
        // whatever the device decides, the map changes buffers and frame slots: both stay the host's to know
        l.front ^= 1;
        at ^= 1;
    }
    launch_follow_shift(reinterpret_cast<const FollowEntry*>(slot.device), bh->d_follow_rects, n, max_cells, bh->d_grid_rows, bh->B, bh->stream);
    launch_inflate_rects(bh->d_follow_rects, n * kFollowRects, max_tiles, bh->stream);
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));   // (after the second launch; only the first reads the slot)
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_follow(ccv_mppi_batch* bh, int32_t* status, int32_t* shift, int64_t* offset, double* origin) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->follow) return fail(bh, CCV_MPPI_ERR_STATE, kNoFollow);
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = follow_refresh(bh)) return rc;
    const size_t n_maps = bh->grid_maps.size();
    std::vector<int32_t> rows(n_maps * kFollowResultInts);
    HIP_TRY(bh, hipMemcpy(rows.data(), bh->d_follow_result, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n_maps; ++m) {
        const int32_t* r = &rows[m * kFollowResultInts];
        if (status) status[m] = r[0];
        if (shift) std::memcpy(shift + 2 * m, r + 1, 2 * sizeof(int32_t));
        if (offset) {
            offset[2 * m] = bh->layers[m].cx;
            offset[2 * m + 1] = bh->layers[m].cy;
        }
        if (origin) {
            origin[2 * m] = bh->grid_maps[m].origin_x;
            origin[2 * m + 1] = bh->grid_maps[m].origin_y;
        }
    }
    return CCV_MPPI_OK;
}

}  // extern "C"

// C ABI, batch handles: the maps of the grid term -- a caller's float cells (ccv_mppi_batch_set_grids) or costmaps derived on the
// device from occupancy layers (_set_occupancy; mppi_costmap.h), and what changes those layers in stream order: patches, rolls
// and range scans, and the simulated range sensor with its world (struct ccv_mppi_batch and its parts Grids, Costmap and World:
// capi_internal.h).  Two shapes.  The setters have
// capi_batch_config.hip's: validate (every check before anything changes), quiesce, commit the host-side state, sync_tables.
// The *_enqueue calls: validate, take a slot of the staging ring (Staging), fill it, launch, seal it -- no flush of the deferred
// resident update (it reads no map), no allocation after the handle's first roll, no wait but for the launches that last read the slot.
#include "capi_internal.h"
#include "mppi_costmap_rects.h"
#include "mppi_costmap_roll.h"
#include "mppi_costmap_scan.h"
#include "mppi_costmap_sense.h"
#include "mppi_costmap_follow.h"

namespace ccv {

float* cells_of(const ccv_mppi_batch* bh, const int m, const bool back) {
    const bool second = bh->occ && ((bh->layers[(size_t)m].front != 0) != back);
    return (second ? bh->d_cells_roll : bh->d_grid_cells) + bh->grid_offset[(size_t)m];
}

uint8_t* layer_of(const ccv_mppi_batch* bh, const int m, const bool back) {
    return ((bh->layers[(size_t)m].front != 0) != back ? bh->d_occ_roll : bh->d_occ) + bh->grid_offset[(size_t)m];
}

// (every cell of the second set that is read later is written first: a shift writes every layer cell, and the shift and the bands
// every float cell)
int ensure_roll_buffers(ccv_mppi_batch* bh) {
    if (bh->d_occ_roll) return CCV_MPPI_OK;
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    const ccv_mppi_grid& last = bh->grid_maps.back();
    const size_t total = bh->grid_offset.back() + (size_t)last.nx * (size_t)last.ny;
    DeviceArray<uint8_t> layers;
    DeviceArray<float> cells;
    hipError_t e = layers.alloc(total);
    if (e == hipSuccess) e = cells.alloc(total);
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "roll_occupancy: allocating the second set of layers and cells", e);
    bh->d_occ_roll = std::move(layers);
    bh->d_cells_roll = std::move(cells);
    return CCV_MPPI_OK;
}

}  // namespace ccv

namespace {

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
    bh->d_grid_cells.reset();
    bh->drop_layers();
    bh->drop_follow();   // (the frames spoke of the old layers too)
    bh->drop_world();   // (the anchors spoke of the old layers)
    bh->grid = false;
    bh->grid_maps.clear();
    bh->grid_offset.clear();
    bh->grid_map_of.clear();
    bh->grid_w.clear();
    return sync_tables(bh);
}

// A new set of maps takes the place of the old one (the caller has quiesced and filled `cells` at `offset`): the grid rows, the
// host copies, the old cells freed.  `cells` is taken on success and only then; on a failure it stays the caller's, whose local
// frees it.  geo: the maps' geometry, cells null.
int install_maps(ccv_mppi_batch* bh, std::vector<ccv_mppi_grid>& geo, DeviceArray<float>&& cells, std::vector<size_t>& offset, const int32_t* map_of,
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
    hipError_t e = bh->d_grid_rows ? hipSuccess : bh->d_grid_rows.alloc((size_t)B);
    if (e == hipSuccess) e = hipMemcpy(bh->d_grid_rows, rows.data(), rows.size() * sizeof(GridRow), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "the grid rows", e);
    bh->d_grid_cells = std::move(cells);
    bh->grid_maps.swap(geo);
    bh->grid_offset.swap(offset);
    bh->grid_map_of.assign(map_of, map_of + B);
    bh->grid_w.assign(weight, weight + B);
    bh->grid = true;
    return CCV_MPPI_OK;
}

// one inflation of the rectangle r inside map m: the float cells from the layer, both the front ones or both the back ones
InflateArgs inflate_args(const ccv_mppi_batch* bh, const int m, const Rect& r, const bool back = false) {
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
    const Costmap::Layer& l = bh->layers[(size_t)m];
    return InflateArgs{layer_of(bh, m, back), cells_of(bh, m, back), bh->d_profile + l.profile_offset, l.free_value, g.nx, g.ny, l.threshold,
                       l.radius, r.x0, r.y0, r.w, r.h};
}

// ... of the float cells that changed layer cells in [x0, x1) x [y0, y1) of map m can move (grown_rect over the map's R)
InflateArgs grown_args(const ccv_mppi_batch* bh, const int m, const int64_t x0, const int64_t y0, const int64_t x1, const int64_t y1) {
    return inflate_args(bh, m, grown_rect(x0, y0, x1, y1, bh->layers[(size_t)m].radius, bh->grid_maps[(size_t)m].nx, bh->grid_maps[(size_t)m].ny));
}

static_assert(kRollBands == kRollMaxRects, "a roll's bands and the rectangles its slot has room for");
// a slot holds an entry table and, directly after it, a table of another type: the second starts aligned whatever the count
static_assert(sizeof(RollEntry) % alignof(InflateArgs) == 0, "a roll's rectangles follow its entries");
static_assert(sizeof(ScanEntry) % alignof(InflateArgs) == 0, "a scan's rectangles follow its entries");
static_assert(sizeof(SenseEntry) % alignof(int32_t) == 0, "a sensing's beams follow its entries");

}  // namespace

extern "C" {

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
    // the cells of all maps are one allocation, sized by the maps: a new set is a new one, the old one goes when that is filled
    DeviceArray<float> cells;
    HIP_TRY(bh, cells.alloc(total));
    std::vector<size_t> offset((size_t)n_maps);
    size_t at = 0;
    for (int m = 0; m < n_maps; ++m) {
        const size_t n = (size_t)maps[m].nx * (size_t)maps[m].ny;
        const hipError_t e = hipMemcpy(cells + at, maps[m].cells, n * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "set_grids: copying the cells", e);
        offset[(size_t)m] = at;
        at += n;
    }
    std::vector<ccv_mppi_grid> geo(maps, maps + n_maps);
    for (ccv_mppi_grid& g : geo) g.cells = nullptr;
    if (int rc = install_maps(bh, geo, std::move(cells), offset, map_of, weight)) return rc;
    bh->drop_layers();   // (the cells are the caller's now)
    bh->drop_follow();
    bh->drop_world();   // (the anchors spoke of the old layers)
    return sync_tables(bh);
}

int ccv_mppi_batch_get_grids(ccv_mppi_batch* bh, ccv_mppi_grid* maps, int32_t max_maps, int32_t* n_maps, int32_t* map_of, double* weight) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int n = bh->grid ? (int)bh->grid_maps.size() : 0;
    if (maps && (max_maps < 0 || max_maps < n)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_grids: max_maps below the number of maps");
    if (bh->follow && maps)
        if (int rc = follow_refresh(bh)) return rc;   // (the origins are the device's)
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
    HIP_TRY(bh, staging_create(bh));
    // cells, layers and profile tables of all maps: three allocations sized by the maps, filled before the old ones go
    DeviceArray<float> cells, profiles;
    DeviceArray<uint8_t> layers;
    std::vector<size_t> offset((size_t)n_maps);
    std::vector<Costmap::Layer> recs((size_t)n_maps);
    hipError_t e = cells.alloc(total);
    if (e == hipSuccess) e = layers.alloc(total);
    if (e == hipSuccess) e = profiles.alloc(n_profile);
    size_t at = 0, pat = 0;
    for (int m = 0; m < n_maps && e == hipSuccess; ++m) {
        const size_t n = (size_t)maps[m].nx * (size_t)maps[m].ny, np = (size_t)inflation[m].radius * (size_t)inflation[m].radius + 1;
        e = hipMemcpy(layers + at, maps[m].cells, n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(profiles + pat, inflation[m].profile, np * sizeof(float), hipMemcpyHostToDevice);
        offset[(size_t)m] = at;
        // (no roll yet: the map in the first allocation, no cell moved; the second allocation goes with the old layers)
        recs[(size_t)m] = Costmap::Layer{pat, maps[m].threshold, inflation[m].radius, inflation[m].free_value, 0, 0, 0, maps[m].origin_x, maps[m].origin_y};
        at += n;
        pat += np;
    }
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "set_occupancy: allocating or copying the layers", e);
    std::vector<ccv_mppi_grid> geo((size_t)n_maps);
    for (int m = 0; m < n_maps; ++m)
        geo[(size_t)m] = ccv_mppi_grid{maps[m].origin_x, maps[m].origin_y, maps[m].resolution, maps[m].outside, maps[m].nx, maps[m].ny, nullptr};
    if (int rc = install_maps(bh, geo, std::move(cells), offset, map_of, weight)) return rc;
    bh->drop_layers();
    bh->drop_follow();
    bh->drop_world();   // (the anchors spoke of the old layers)
    bh->d_occ = std::move(layers);
    bh->d_profile = std::move(profiles);
    bh->layers.swap(recs);
    bh->occ = true;
    // one full inflation per map; the stream is idle again before the tables point at the cells
    for (int m = 0; m < n_maps; ++m) launch_inflate(inflate_args(bh, m, Rect{0, 0, maps[m].nx, maps[m].ny}), bh->stream);
    HIP_TRY(bh, hipGetLastError());
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));
    return sync_tables(bh);
}

// Two launches: no workgroup of the inflation reads a layer cell another is writing.  The inflation does not read the slot.
int ccv_mppi_batch_update_occupancy_enqueue(ccv_mppi_batch* bh, int32_t map, int32_t x0, int32_t y0, int32_t w, int32_t h, const uint8_t* patch) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "update_occupancy: ";
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "update_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (!patch) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (map < 0 || map >= (int32_t)bh->grid_maps.size()) return refuse(bh, who, "map out of range");
    const ccv_mppi_grid& g = bh->grid_maps[(size_t)map];
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || w > g.nx - x0 || h > g.ny - y0) return refuse(bh, who, "the rectangle is not inside the map");
    if ((int64_t)w * h > CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "more than CCV_MPPI_OCC_PATCH_MAX_CELLS cells");
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    std::memcpy(slot.host, patch, (size_t)w * (size_t)h);
    launch_occupancy_patch(layer_of(bh, map), g.nx, slot.device, x0, y0, w, h, bh->stream);
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));
    launch_inflate(grown_args(bh, map, x0, y0, (int64_t)x0 + w, (int64_t)y0 + h), bh->stream);
    HIP_TRY(bh, hipGetLastError());
    return CCV_MPPI_OK;
}

// The handle's first roll allocates the second set of layers and cells, and quiesces for it like a setter.  Two launches in all.
int ccv_mppi_batch_roll_occupancy_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* map, const int32_t* dx, const int32_t* dy,
                                          const uint8_t* exposed, int32_t fill) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "roll_occupancy: ";
    // every check comes before anything changes
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "roll_occupancy: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (bh->follow) return fail(bh, CCV_MPPI_ERR_STATE, "roll_occupancy: the maps follow their robots (ccv_mppi_batch_resident_set_follow): the windows are the device's to move");
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
        if (const char* fault = name_fault(named, m)) return refuse(bh, who, fault);
        const int64_t ex = dx[i], ey = dy[i];
        if (ex < -CCV_MPPI_GRID_MAX_DIM || ex > CCV_MPPI_GRID_MAX_DIM || ey < -CCV_MPPI_GRID_MAX_DIM || ey > CCV_MPPI_GRID_MAX_DIM)
            return refuse(bh, who, "|dx| or |dy| above CCV_MPPI_GRID_MAX_DIM");
        const Costmap::Layer& l = bh->layers[(size_t)m];
        const int64_t cx = l.cx + ex, cy = l.cy + ey;
        if (cx < -kMaxOffset || cx > kMaxOffset || cy < -kMaxOffset || cy > kMaxOffset)
            return refuse(bh, who, "an accumulated offset beyond 2^30 cells");
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        // (from the accumulated cell count, one product and one sum: no drift, and a checker can restate it exactly)
        ox[(size_t)i] = l.ox0 + (double)cx * g.resolution;
        oy[(size_t)i] = l.oy0 + (double)cy * g.resolution;
        if (!std::isfinite(ox[(size_t)i]) || !std::isfinite(oy[(size_t)i])) return refuse(bh, who, "a rolled origin is not finite");
        if (ex == 0 && ey == 0) continue;
        ++moved;
        if (exposed) strip_bytes += roll_exposed_cells(g.nx, g.ny, ex, ey);
    }
    const size_t entry_bytes = moved * sizeof(RollEntry), rect_bytes = moved * kRollMaxRects * sizeof(InflateArgs);
    if (entry_bytes + rect_bytes + strip_bytes > (size_t)CCV_MPPI_OCC_PATCH_MAX_CELLS)
        return refuse(bh, who, "tables and strips above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    // the second set of layers and cells, at the handle's first roll since the layers were set
    if (int rc = ensure_roll_buffers(bh)) return rc;
    if (moved == 0) return CCV_MPPI_OK;   // (nothing moves: no launch, no bit changes)
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    // the slot: the entries, the rectangles, the strips (the kernels read all three in place)
    RollEntry* entries = reinterpret_cast<RollEntry*>(slot.host);
    InflateArgs* rects = reinterpret_cast<InflateArgs*>(slot.host + entry_bytes);
    uint8_t* strips = slot.host + entry_bytes + rect_bytes;
    const uint8_t* d_strips = slot.device + entry_bytes + rect_bytes;
    size_t n_entries = 0, n_rects = 0, strip_at = 0;
    int64_t max_cells = 0;
    int32_t max_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const int m = map[i], ex = dx[i], ey = dy[i];
        if (ex == 0 && ey == 0) continue;
        ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        Costmap::Layer& l = bh->layers[(size_t)m];
        const size_t bytes = exposed ? roll_exposed_cells(g.nx, g.ny, ex, ey) : 0;
        if (bytes) std::memcpy(strips + strip_at, exposed + strip_at, bytes);
        entries[n_entries++] = RollEntry{layer_of(bh, m), layer_of(bh, m, true), cells_of(bh, m), cells_of(bh, m, true),
                                         exposed ? d_strips + strip_at : nullptr, ox[(size_t)i], oy[(size_t)i], g.nx, g.ny, ex, ey, fill, 0};
        strip_at += bytes;
        max_cells = std::max<int64_t>(max_cells, (int64_t)g.nx * g.ny);
        Rect band[kRollMaxRects];
        const int n_bands = roll_bands(g.nx, g.ny, ex, ey, l.radius, band);
        for (int k = 0; k < n_bands; ++k) {
            rects[n_rects++] = inflate_args(bh, m, band[k], true);
            max_tiles = std::max(max_tiles, inflate_tiles(band[k].w, band[k].h));
        }
        // the host's view moves at call time: the front bit, the offsets, the origin _get_grids and _get_occupancy return
        l.front ^= 1;
        l.cx += ex;
        l.cy += ey;
        g.origin_x = ox[(size_t)i];
        g.origin_y = oy[(size_t)i];
    }
    launch_roll_shift(reinterpret_cast<const RollEntry*>(slot.device), (int32_t)n_entries, max_cells, bh->d_grid_rows, bh->B, bh->stream);
    launch_inflate_rects(reinterpret_cast<const InflateArgs*>(slot.device + entry_bytes), (int32_t)n_rects, max_tiles, bh->stream);
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));   // (after the second launch: both read the slot)
    return CCV_MPPI_OK;
}

// Two launches however many maps are scanned; the front buffers are written in place (Layer::front, the grid rows: untouched).
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
        if (const char* fault = name_fault(named, m)) return refuse(bh, who, fault);
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
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    // the slot: the entries, the rectangles, the end cells, the hit bytes (the kernels read all four in place)
    const size_t end_at = entry_bytes + rect_bytes, hit_at = end_at + (size_t)total * 2 * sizeof(int32_t);
    ScanEntry* entries = reinterpret_cast<ScanEntry*>(slot.host);
    InflateArgs* rects = reinterpret_cast<InflateArgs*>(slot.host + entry_bytes);
    std::memcpy(slot.host + end_at, end_xy, (size_t)total * 2 * sizeof(int32_t));
    std::memcpy(slot.host + hit_at, hit, (size_t)total);
    const int32_t* d_end = reinterpret_cast<const int32_t*>(slot.device + end_at);
    const uint8_t* d_hit = slot.device + hit_at;
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
        // the float cells to derive again: the box holds every cell the entry can change
        const int64_t* bb = &box[(size_t)i * 4];
        const InflateArgs a = grown_args(bh, m, bb[0], bb[1], bb[2] + 1, bb[3] + 1);
        rects[k++] = a;
        max_tiles = std::max(max_tiles, inflate_tiles(a.w, a.h));
    }
    launch_scan_trace(reinterpret_cast<const ScanEntry*>(slot.device), (int32_t)traced, bh->stream);
    launch_inflate_rects(reinterpret_cast<const InflateArgs*>(slot.device + entry_bytes), (int32_t)traced, max_tiles, bh->stream);
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));   // (after the second launch: both read the slot)
    return CCV_MPPI_OK;
}

// ---- the simulated range sensor: a ground-truth world, and the resident robots' beams cast through it (mppi_costmap_sense.h) ----

int ccv_mppi_batch_set_world(ccv_mppi_batch* bh, const ccv_mppi_occupancy* world, const int32_t* anchor_xy, int32_t max_beams) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "set_world: ";
    if (!world) {
        if (!bh->world) return CCV_MPPI_OK;
        const DeviceGuard guard(bh->cfg.device);
        if (int rc = quiesce(bh)) return rc;   // (a queued sensing may still read the world and write the read-back)
        bh->drop_world();
        return CCV_MPPI_OK;
    }
    // every check comes before anything changes
    if (!bh->occ) return fail(bh, CCV_MPPI_ERR_STATE, "set_world: no occupancy is set (ccv_mppi_batch_set_occupancy)");
    if (!world->cells || !anchor_xy) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (const char* fault = geometry_fault(world->nx, world->ny, world->resolution, world->origin_x, world->origin_y, 0.0f)) return refuse(bh, who, fault);
    if (world->threshold < 0 || world->threshold > 255) return refuse(bh, who, "a threshold outside [0, 255]");
    if (max_beams < 1 || max_beams > CCV_MPPI_SENSE_MAX_BEAMS) return refuse(bh, who, "max_beams outside [1, CCV_MPPI_SENSE_MAX_BEAMS]");
    const size_t n_maps = bh->grid_maps.size();
    constexpr int32_t kMaxAnchor = 1 << 29;
    for (size_t i = 0; i < 2 * n_maps; ++i)
        if (anchor_xy[i] < -kMaxAnchor || anchor_xy[i] > kMaxAnchor) return refuse(bh, who, "an anchor beyond 2^29 cells");
    const DeviceGuard guard(bh->cfg.device);
    if (int rc = quiesce(bh)) return rc;
    // the world, the read-back and the rectangle table: four allocations, filled before the old ones go
    const size_t cells = (size_t)world->nx * (size_t)world->ny, first_bytes = (size_t)bh->B * (size_t)max_beams * sizeof(int32_t);
    const size_t cell_bytes = (size_t)bh->B * 2 * sizeof(int32_t);
    DeviceArray<uint8_t> layer;
    DeviceArray<int32_t> first, sensor;
    DeviceArray<InflateArgs> rects;
    hipError_t e = layer.alloc(cells);
    if (e == hipSuccess) e = first.alloc(first_bytes / sizeof(int32_t));
    if (e == hipSuccess) e = sensor.alloc(cell_bytes / sizeof(int32_t));
    if (e == hipSuccess) e = rects.alloc((size_t)bh->B);
    if (e == hipSuccess) e = hipMemcpy(layer, world->cells, cells, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(first, 0xFF, first_bytes, bh->stream);   // (-1: no beam blocked, nothing sensed)
    if (e == hipSuccess) e = hipMemsetAsync(sensor, 0xFF, cell_bytes, bh->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rects, 0, (size_t)bh->B * sizeof(InflateArgs), bh->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(bh->stream);
    if (e != hipSuccess) return fail(bh, CCV_MPPI_ERR_HIP, "set_world: allocating or copying the world", e);
    bh->drop_world();
    bh->d_world = std::move(layer);
    bh->d_sense_first = std::move(first);
    bh->d_sense_cell = std::move(sensor);
    bh->d_sense_rects = std::move(rects);
    bh->world_geo = *world;
    bh->world_geo.cells = nullptr;
    bh->world_anchor.assign(anchor_xy, anchor_xy + 2 * n_maps);
    bh->world_max_beams = max_beams;
    bh->world = true;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_get_world(ccv_mppi_batch* bh, ccv_mppi_occupancy* world, int32_t* anchor_xy, int32_t max_maps, int32_t* max_beams) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->world) return fail(bh, CCV_MPPI_ERR_STATE, "get_world: no world is set (ccv_mppi_batch_set_world)");
    if (anchor_xy && (max_maps < 0 || (size_t)max_maps < bh->grid_maps.size())) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_world: max_maps below the number of maps");
    if (world) *world = bh->world_geo;
    if (anchor_xy) std::memcpy(anchor_xy, bh->world_anchor.data(), bh->world_anchor.size() * sizeof(int32_t));
    if (max_beams) *max_beams = bh->world_max_beams;
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_read_world(ccv_mppi_batch* bh, uint8_t* out) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!out) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (!bh->world) return fail(bh, CCV_MPPI_ERR_STATE, "read_world: no world is set (ccv_mppi_batch_set_world)");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued patch writers)
    HIP_TRY(bh, hipMemcpy(out, bh->d_world, (size_t)bh->world_geo.nx * (size_t)bh->world_geo.ny, hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}

// One launch: the patch writer on the world layer.  Nothing is derived from the world; the next sensing reads the new cells.
int ccv_mppi_batch_update_world_enqueue(ccv_mppi_batch* bh, int32_t x0, int32_t y0, int32_t w, int32_t h, const uint8_t* patch) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "update_world: ";
    if (!bh->world) return fail(bh, CCV_MPPI_ERR_STATE, "update_world: no world is set (ccv_mppi_batch_set_world)");
    if (!patch) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    const ccv_mppi_occupancy& g = bh->world_geo;
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || w > g.nx - x0 || h > g.ny - y0) return refuse(bh, who, "the rectangle is not inside the world");
    if ((int64_t)w * h > CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "more than CCV_MPPI_OCC_PATCH_MAX_CELLS cells");
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    std::memcpy(slot.host, patch, (size_t)w * (size_t)h);
    launch_occupancy_patch(bh->d_world, g.nx, slot.device, x0, y0, w, h, bh->stream);
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));
    return CCV_MPPI_OK;
}

// Two launches however many robots sense: the beams (k_sense_trace, which also writes the rectangles into device memory) and
// the inflation of those rectangles.  The poses are the device's: nothing here reads one.
int ccv_mppi_batch_resident_sense_enqueue(ccv_mppi_batch* bh, int32_t n, const int32_t* instance, int32_t n_beams, const int32_t* beam_xy,
                                          int32_t clear_value, int32_t mark_value) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    static const char who[] = "resident_sense: ";
    // every check comes first, then the next slot of the ring
    if (!bh->world) return fail(bh, CCV_MPPI_ERR_STATE, "resident_sense: no world is set (ccv_mppi_batch_set_world)");
    if (!bh->have_paths || !bh->have_poses) return fail(bh, CCV_MPPI_ERR_STATE, "resident_sense: ccv_mppi_batch_resident_set_paths and _set_poses first");
    if (!instance || !beam_xy) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "null pointer argument");
    if (n < 1 || n > bh->B) return refuse(bh, who, "n outside [1, B]");
    if (n_beams < 1 || n_beams > bh->world_max_beams) return refuse(bh, who, "n_beams outside [1, max_beams]");
    if (clear_value < 0 || clear_value > 255 || mark_value < 0 || mark_value > 255) return refuse(bh, who, "clear_value or mark_value outside [0, 255]");
    const size_t entry_bytes = (size_t)n * (bh->follow ? sizeof(SenseFollowEntry) : sizeof(SenseEntry)), beam_bytes = (size_t)n_beams * 2 * sizeof(int32_t);
    if (entry_bytes + beam_bytes > (size_t)CCV_MPPI_OCC_PATCH_MAX_CELLS) return refuse(bh, who, "entries and beams above a staging slot (CCV_MPPI_OCC_PATCH_MAX_CELLS bytes)");
    constexpr int64_t kMaxOffset = (int64_t)1 << 30;
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
        if (std::memcmp(&bh->grid_maps[(size_t)m].resolution, &bh->world_geo.resolution, sizeof(double)) != 0)
            return refuse(bh, who, "a map's resolution differs from the world's");
        if (bh->follow) continue;   // (the rolled count is the device's: at most 2^30 there, and the anchor at most 2^29)
        const Costmap::Layer& l = bh->layers[(size_t)m];
        const int64_t ox = bh->world_anchor[2 * (size_t)m] + l.cx, oy = bh->world_anchor[2 * (size_t)m + 1] + l.cy;
        if (ox < -kMaxOffset || ox > kMaxOffset || oy < -kMaxOffset || oy > kMaxOffset) return refuse(bh, who, "a frame offset beyond 2^30 cells");
    }
    SenseArgs A{};
    // (the extent of the beam table starts from the offset (0, 0): the box holds the sensor cell and every end cell)
    for (int r = 0; r < n_beams; ++r) {
        const int32_t dx = beam_xy[2 * (size_t)r], dy = beam_xy[2 * (size_t)r + 1];
        if (dx < -CCV_MPPI_SCAN_MAX_REACH || dx > CCV_MPPI_SCAN_MAX_REACH || dy < -CCV_MPPI_SCAN_MAX_REACH || dy > CCV_MPPI_SCAN_MAX_REACH)
            return refuse(bh, who, "a reach above CCV_MPPI_SCAN_MAX_REACH");
        A.min_dx = std::min(A.min_dx, dx);
        A.max_dx = std::max(A.max_dx, dx);
        A.min_dy = std::min(A.min_dy, dy);
        A.max_dy = std::max(A.max_dy, dy);
    }
    Slot slot;
    HIP_TRY(bh, bh->ring.take(slot));
    // the slot: the entries, the beams (the kernel reads both in place).  While the maps follow, the entries carry the anchor and
    // the address of the map's frame, and one small launch completes them in device memory (mppi_costmap_follow.h)
    SenseEntry* entries = reinterpret_cast<SenseEntry*>(slot.host);
    SenseFollowEntry* followed = reinterpret_cast<SenseFollowEntry*>(slot.host);
    std::memcpy(slot.host + entry_bytes, beam_xy, beam_bytes);
    const ccv_mppi_occupancy& w = bh->world_geo;
    A.world = bh->d_world;
    A.beam_xy = reinterpret_cast<const int32_t*>(slot.device + entry_bytes);
    A.origin_x = w.origin_x;
    A.origin_y = w.origin_y;
    A.inv = 1.0 / w.resolution;
    A.wnx = w.nx;
    A.wny = w.ny;
    A.threshold = w.threshold;
    A.n_beams = n_beams;
    A.clear_value = clear_value;
    A.mark_value = mark_value;
    const int32_t span_x = A.max_dx - A.min_dx + 1, span_y = A.max_dy - A.min_dy + 1;
    int32_t max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        const int b = instance[i], m = bh->grid_map_of[(size_t)b];
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        const Costmap::Layer& l = bh->layers[(size_t)m];
        SenseEntry& e = bh->follow ? followed[i].entry : entries[i];
        e.rect = inflate_args(bh, m, Rect{0, 0, 0, 0});
        e.layer = layer_of(bh, m);
        e.pose = bh->d_rframe[b].x0;   // (an address: the host reads no pose)
        e.first = bh->d_sense_first + (size_t)b * (size_t)bh->world_max_beams;
        e.sensor_cell = bh->d_sense_cell + 2 * (size_t)b;
        e.pad[0] = e.pad[1] = 0;
        if (bh->follow) {   // (the anchor alone: the device adds the cells the map has rolled)
            e.off_x = bh->world_anchor[2 * (size_t)m];
            e.off_y = bh->world_anchor[2 * (size_t)m + 1];
            followed[i].frame = bh->d_follow_frames + 2 * (size_t)m + bh->follow_slot[(size_t)m];
            followed[i].pad = 0;
        } else {
            e.off_x = (int32_t)(bh->world_anchor[2 * (size_t)m] + l.cx);
            e.off_y = (int32_t)(bh->world_anchor[2 * (size_t)m + 1] + l.cy);
        }
        // the largest rectangle the device can form: the box clipped to the map, grown by R and clipped again
        max_tiles = std::max(max_tiles, inflate_tiles(std::min(g.nx, span_x + 2 * l.radius), std::min(g.ny, span_y + 2 * l.radius)));
    }
    if (bh->follow) {
        launch_follow_resolve_sense(reinterpret_cast<const SenseFollowEntry*>(slot.device), bh->d_follow_sense, n, bh->stream);
        launch_sense_trace(bh->d_follow_sense, bh->d_sense_rects, n, A, bh->stream);
    } else {
        launch_sense_trace(reinterpret_cast<const SenseEntry*>(slot.device), bh->d_sense_rects, n, A, bh->stream);
    }
    launch_inflate_rects(bh->d_sense_rects, n, max_tiles, bh->stream);
    // (after the last launch; the beam kernel reads the slot, and while the maps follow the launch ahead of it does too)
    HIP_TRY(bh, bh->ring.seal(slot, hipGetLastError(), bh->stream));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_resident_read_sense(ccv_mppi_batch* bh, int32_t* first, int32_t* sensor_cell) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    if (!bh->world) return fail(bh, CCV_MPPI_ERR_STATE, "resident_read_sense: no world is set (ccv_mppi_batch_set_world)");
    const DeviceGuard guard(bh->cfg.device);
    HIP_TRY(bh, hipSetDevice(bh->cfg.device));
    HIP_TRY(bh, hipStreamSynchronize(bh->stream));   // (queued sensings)
    if (first) HIP_TRY(bh, hipMemcpy(first, bh->d_sense_first, (size_t)bh->B * (size_t)bh->world_max_beams * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sensor_cell) HIP_TRY(bh, hipMemcpy(sensor_cell, bh->d_sense_cell, (size_t)bh->B * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CCV_MPPI_OK;
}

int ccv_mppi_batch_get_occupancy(ccv_mppi_batch* bh, ccv_mppi_occupancy* maps, ccv_mppi_inflation* inflation, int32_t max_maps, int32_t* n_maps) {
    if (!bh) return CCV_MPPI_ERR_INVALID_ARG;
    const int n = bh->occ ? (int)bh->grid_maps.size() : 0;
    if ((maps || inflation) && (max_maps < 0 || max_maps < n)) return fail(bh, CCV_MPPI_ERR_INVALID_ARG, "get_occupancy: max_maps below the number of maps");
    if (bh->follow && maps)
        if (int rc = follow_refresh(bh)) return rc;   // (the origins are the device's)
    if (n_maps) *n_maps = n;
    for (int m = 0; m < n; ++m) {
        const ccv_mppi_grid& g = bh->grid_maps[(size_t)m];
        if (maps) maps[m] = ccv_mppi_occupancy{g.origin_x, g.origin_y, g.resolution, g.outside, g.nx, g.ny, bh->layers[(size_t)m].threshold, nullptr};
        if (inflation) inflation[m] = ccv_mppi_inflation{bh->layers[(size_t)m].radius, bh->layers[(size_t)m].free_value, nullptr};
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

}  // extern "C"

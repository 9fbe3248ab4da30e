// Host arithmetic of the costmap calls (capi_batch_maps.hip) that needs neither a handle nor a device: the rectangles of float
// cells a patch, a scan and a roll derive again, a roll's exposed cells, and the check that a call names a map once.  Integers
// and the standard library only, so that a stand-alone host program can run it (tools/costmap_rects_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

// (roll_bands also runs in k_costmap_follow.hip: one statement for the host's rolls and the device's)
#ifdef __HIPCC__
#define CCV_RECTS_HD __host__ __device__
#else
#define CCV_RECTS_HD
#endif

namespace ccv {

struct Rect { int32_t x0, y0, w, h; };

// A changed layer cell moves the cost of cells up to R away: the cells [x0, x1) x [y0, y1), which meet the map, grown by R and
// clipped to the nx x ny map hold every float cell whose value can change (from layer cells up to 2R from the rectangle).
inline Rect grown_rect(const int64_t x0, const int64_t y0, const int64_t x1, const int64_t y1, const int R, const int32_t nx, const int32_t ny) {
    const int32_t gx0 = (int32_t)std::max<int64_t>(x0 - R, 0), gy0 = (int32_t)std::max<int64_t>(y0 - R, 0);
    const int32_t gx1 = (int32_t)std::min<int64_t>(x1 + R, nx), gy1 = (int32_t)std::min<int64_t>(y1 + R, ny);
    return Rect{gx0, gy0, gx1 - gx0, gy1 - gy0};
}

// the exposed cells of a roll of an nx x ny map by (dx, dy): min(|dy|, ny) full rows, min(|dx|, nx) cells of each remaining row
inline size_t roll_exposed_cells(const int32_t nx, const int32_t ny, const int64_t dx, const int64_t dy) {
    const size_t ax = (size_t)std::min<int64_t>(std::llabs(dx), nx), ay = (size_t)std::min<int64_t>(std::llabs(dy), ny);
    return ay * (size_t)nx + ((size_t)ny - ay) * ax;
}

// The float cells a roll by (ex, ey) derives again: within R of an exposed cell (the leading band, |d| + R
// wide) or of a cell that left the map (the trailing band, R wide), per axis; every other float cell is the shift's copy.  The
// bands in y keep to the columns the bands in x leave: no cell is written twice.  Returns how many of the four are not empty.
constexpr int kRollBands = 4;
CCV_RECTS_HD inline int roll_bands(const int nx, const int ny, const int ex, const int ey, const int R, Rect out[kRollBands]) {
    const int lx = ex ? std::min(std::abs(ex) + R, nx) : 0, tx = ex ? std::min(R, nx - lx) : 0;
    const int ly = ey ? std::min(std::abs(ey) + R, ny) : 0, ty = ey ? std::min(R, ny - ly) : 0;
    const int xa = ex > 0 ? tx : lx, xb = ex > 0 ? nx - lx : nx - tx;   // the columns between the bands in x
    const Rect band[kRollBands] = {{ex > 0 ? nx - lx : 0, 0, lx, ny},
                                   {ex > 0 ? 0 : nx - tx, 0, tx, ny},
                                   {xa, ey > 0 ? ny - ly : 0, xb - xa, ly},
                                   {xa, ey > 0 ? 0 : ny - ty, xb - xa, ty}};
    int n = 0;
    for (const Rect& r : band)
        if (r.w >= 1 && r.h >= 1) out[n++] = r;
    return n;
}

// map m of a call that names maps (named: a zero per map of the handle before the call's first): null, or what is wrong
inline const char* name_fault(std::vector<uint8_t>& named, const int m) {
    if (m < 0 || m >= (int)named.size()) return "map out of range";
    if (named[(size_t)m]) return "a map is named twice";
    named[(size_t)m] = 1;
    return nullptr;
}

}  // namespace ccv

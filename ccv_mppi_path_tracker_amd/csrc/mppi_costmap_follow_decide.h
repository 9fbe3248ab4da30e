// The decision of a costmap that follows its robot (mppi_costmap_follow.h has the statement): whether and
// by how many cells the window moves, and the frame it has afterwards.  Doubles, integers and <cmath> only, so that the kernel
// (k_costmap_follow.hip) and a stand-alone host program (tools/costmap_follow_check.cpp) run the same lines.  Built without
// contraction, as everything here: one rounding per operation.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define CCV_FOLLOW_HD __host__ __device__
#else
#define CCV_FOLLOW_HD
#endif

namespace ccv {

constexpr int kFollowMoved = 1, kFollowHeld = 2, kFollowNoPose = 3, kFollowLimit = 4;   // CCV_MPPI_FOLLOW_*
constexpr int kFollowResultInts = 4;   // a result row: status, dx, dy, 0
constexpr int kFollowRects = 4;        // per entry: kRollBands (mppi_costmap_rects.h)

// a map's frame: the cells moved since _set_occupancy and the origin that goes with them
struct FollowFrame {
    int64_t cx, cy;
    double origin_x, origin_y;
};
static_assert(sizeof(FollowFrame) == 32, "two slots per map in one table");

struct FollowDecision {
    int32_t status, dx, dy;
    FollowFrame frame;   // the frame after the call: the old one unless status is MOVED
};

CCV_FOLLOW_HD inline FollowDecision follow_decide(const double x, const double y, const FollowFrame& f, const double ox0, const double oy0,
                                                        const double resolution, const double inv, const int32_t nx, const int32_t ny,
                                                        const int32_t margin, const int32_t max_step) {
    constexpr double kLimit = 1073741824.0;   // 2^30
    constexpr int64_t kMaxOffset = (int64_t)1 << 30;
    FollowDecision d{kFollowNoPose, 0, 0, f};
    const double fx = (x - f.origin_x) * inv, fy = (y - f.origin_y) * inv;
    if (!(fabs(fx) < kLimit && fabs(fy) < kLimit)) return d;
    const int64_t ex = (int64_t)floor(fx) - nx / 2, ey = (int64_t)floor(fy) - ny / 2;
    const int64_t ax = ex < 0 ? -ex : ex, ay = ey < 0 ? -ey : ey;
    const int64_t dx = ax <= margin ? 0 : (ex < -max_step ? -max_step : ex > max_step ? max_step : ex);
    const int64_t dy = ay <= margin ? 0 : (ey < -max_step ? -max_step : ey > max_step ? max_step : ey);
    d.status = kFollowHeld;
    if (dx == 0 && dy == 0) return d;
    d.status = kFollowLimit;
    const int64_t cx = f.cx + dx, cy = f.cy + dy;
    if (cx < -kMaxOffset || cx > kMaxOffset || cy < -kMaxOffset || cy > kMaxOffset) return d;
    const double ox = ox0 + (double)cx * resolution, oy = oy0 + (double)cy * resolution;
    if (!(fabs(ox) <= 1.7976931348623157e308 && fabs(oy) <= 1.7976931348623157e308)) return d;
    d.status = kFollowMoved;
    d.dx = (int32_t)dx;
    d.dy = (int32_t)dy;
    d.frame = FollowFrame{cx, cy, ox, oy};
    return d;
}

}  // namespace ccv

// Stand-alone host check of csrc/mppi_costmap_rects.h and of inflate_tiles (csrc/mppi_costmap.h): no device, no library.  Meant
// to be built with the address and undefined-behaviour sanitizers and run once:
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__
//         -I$ROCM_PATH/include -Iccv_mppi_path_tracker_amd/csrc tools/costmap_rects_check.cpp -o costmap_rects_check
//   ./costmap_rects_check
// (mppi_costmap.h names hipStream_t, hence the HIP include path; nothing of HIP is called or linked for its sake.)
// The bands of a roll are held against the statement of tests/roll_reference.py (roll_bands, restated in reference_bands below):
// the same set of cells, and no cell in two of the four rectangles.  Exits non-zero if anything differs.
#include <cstdio>
#include <string>
#include <vector>

#include "mppi_costmap.h"
#include "mppi_costmap_rects.h"

using namespace ccv;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
            ++failures;                        \
        }                                      \
    } while (0)

// tests/roll_reference.py, roll_bands with lead = trail = R: per moving axis a leading band of min(|d| + R, n) cells on the side
// the exposed cells appear and a trailing band of min(R, n) cells on the other, over the full other axis; they may overlap
static std::vector<Rect> reference_bands(const int nx, const int ny, const int dx, const int dy, const int R) {
    std::vector<Rect> out;
    for (int axis = 0; axis < 2; ++axis) {
        const int n = axis == 0 ? nx : ny, d = axis == 0 ? dx : dy;
        if (d == 0) continue;
        const int wl = std::min(std::abs(d) + R, n), wt = std::min(R, n);
        const int lo[2] = {d > 0 ? n - wl : 0, d > 0 ? 0 : n - wt}, w[2] = {wl, wt};
        for (int k = 0; k < 2; ++k)
            if (w[k] > 0) out.push_back(axis == 0 ? Rect{lo[k], 0, w[k], ny} : Rect{0, lo[k], nx, w[k]});
    }
    return out;
}

static void paint(std::vector<int>& cells, const int nx, const int ny, const Rect& r) {
    CHECK(r.w >= 1 && r.h >= 1 && r.x0 >= 0 && r.y0 >= 0 && r.x0 + r.w <= nx && r.y0 + r.h <= ny, "rectangle (%d, %d, %d, %d) in %d x %d", r.x0,
          r.y0, r.w, r.h, nx, ny);
    for (int y = r.y0; y < r.y0 + r.h; ++y)
        for (int x = r.x0; x < r.x0 + r.w; ++x) ++cells.at((size_t)y * nx + x);
}

static void check_roll(const int nx, const int ny, const int dx, const int dy, const int R) {
    Rect band[kRollBands];
    const int n = roll_bands(nx, ny, dx, dy, R, band);
    CHECK(n >= 0 && n <= kRollBands, "%d bands", n);
    std::vector<int> mine((size_t)nx * ny, 0), ref((size_t)nx * ny, 0);
    for (int k = 0; k < n; ++k) paint(mine, nx, ny, band[k]);
    for (const Rect& r : reference_bands(nx, ny, dx, dy, R)) paint(ref, nx, ny, r);
    size_t exposed = 0;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t i = (size_t)y * nx + x;
            CHECK(mine[i] <= 1, "cell (%d, %d) of %d x %d rolled by (%d, %d), R = %d, is in %d bands", x, y, nx, ny, dx, dy, R, mine[i]);
            CHECK((mine[i] > 0) == (ref[i] > 0), "cell (%d, %d) of %d x %d rolled by (%d, %d), R = %d: band %d, reference %d", x, y, nx, ny, dx, dy,
                  R, mine[i], ref[i]);
            const long sx = (long)x + dx, sy = (long)y + dy;
            exposed += !(sx >= 0 && sx < nx && sy >= 0 && sy < ny);
        }
    CHECK(roll_exposed_cells(nx, ny, dx, dy) == exposed, "%d x %d rolled by (%d, %d): %zu exposed cells, counted %zu", nx, ny, dx, dy,
          roll_exposed_cells(nx, ny, dx, dy), exposed);
}

static void check_grown(const int nx, const int ny, const long x0, const long y0, const long x1, const long y1, const int R) {
    const Rect g = grown_rect(x0, y0, x1, y1, R, nx, ny);
    // cell by cell: inside the map and within R of [x0, x1) x [y0, y1) in both axes
    long lo_x = nx, hi_x = -1, lo_y = ny, hi_y = -1;
    for (long x = 0; x < nx; ++x)
        if (x >= x0 - R && x < x1 + R) lo_x = std::min(lo_x, x), hi_x = std::max(hi_x, x);
    for (long y = 0; y < ny; ++y)
        if (y >= y0 - R && y < y1 + R) lo_y = std::min(lo_y, y), hi_y = std::max(hi_y, y);
    CHECK(g.x0 == lo_x && g.w == hi_x - lo_x + 1 && g.y0 == lo_y && g.h == hi_y - lo_y + 1,
          "[%ld, %ld) x [%ld, %ld) grown by %d in %d x %d: (%d, %d, %d, %d), cell by cell (%ld, %ld, %ld, %ld)", x0, x1, y0, y1, R, nx, ny, g.x0,
          g.y0, g.w, g.h, lo_x, lo_y, hi_x - lo_x + 1, hi_y - lo_y + 1);
}

int main() {
    // rolls: maps narrower or lower than R, |d| at and past the map's size, one axis at rest, both signs
    const int sizes[][2] = {{1, 1}, {3, 2}, {5, 70}, {70, 5}, {64, 64}, {65, 67}, {130, 129}, {200, 3}};
    const int radii[] = {0, 1, 4, 64};
    for (const auto& s : sizes)
        for (const int R : radii) {
            const int nx = s[0], ny = s[1];
            const int moves[][2] = {{1, 0}, {0, -1}, {3, -2}, {-64, 5}, {nx - 1, 0}, {nx, 0}, {0, ny}, {nx + 5, -ny}, {32768, 1}, {-1, -32768}, {R, R}, {-R - 1, 0}};
            for (const auto& d : moves)
                for (const int sign : {1, -1})
                    if (d[0] || d[1]) check_roll(nx, ny, sign * d[0], sign * d[1], R);
        }
    Rect none[kRollBands];
    CHECK(roll_bands(7, 9, 0, 0, 3, none) == 0, "a roll by (0, 0) has bands");
    // grown rectangles: a patch in a corner, across the whole map, a scan's box far outside the map on every side
    for (const auto& s : sizes)
        for (const int R : radii) {
            const int nx = s[0], ny = s[1];
            check_grown(nx, ny, 0, 0, 1, 1, R);
            check_grown(nx, ny, nx - 1, ny - 1, nx, ny, R);
            check_grown(nx, ny, 0, 0, nx, ny, R);
            check_grown(nx, ny, nx / 2, ny / 3, nx / 2 + 1, ny / 3 + 1, R);
            check_grown(nx, ny, -4096, -4096, 1, 1, R);
            check_grown(nx, ny, nx - 1, 0, nx + 4096, ny + 4096, R);
            check_grown(nx, ny, -4096, ny / 2, nx + 4096, ny / 2 + 1, R);
        }
    // tiles
    const int ns[] = {1, 63, 64, 65, 128, 129, 32768};
    for (const int w : ns)
        for (const int h : ns) {
            int tiles = 0;
            for (int y = 0; y < h; y += kInflateTile)
                for (int x = 0; x < w; x += kInflateTile) ++tiles;
            CHECK(inflate_tiles(w, h) == tiles && inflate_tiles(w) * inflate_tiles(h) == tiles, "%d x %d: %d tiles, counted %d", w, h, inflate_tiles(w, h), tiles);
        }
    // a map is named once
    std::vector<uint8_t> named(3, 0);
    const int order[] = {2, 0, -1, 3, 2, 1, 1, 0};
    const char* want[] = {nullptr, nullptr, "map out of range", "map out of range", "a map is named twice", nullptr, "a map is named twice", "a map is named twice"};
    for (int i = 0; i < 8; ++i) {
        const char* got = name_fault(named, order[i]);
        CHECK((got == nullptr) == (want[i] == nullptr) && (!got || std::string(got) == want[i]), "naming map %d (step %d): %s", order[i], i, got ? got : "accepted");
    }
    std::vector<uint8_t> empty;
    CHECK(name_fault(empty, 0) != nullptr, "a handle without maps accepted map 0");
    std::printf("%s\n", failures ? "costmap_rects_check: FAILED" : "costmap_rects_check: ok");
    return failures ? 1 : 0;
}

// Stand-alone host run of what the follow kernel decides with (csrc/mppi_costmap_follow_decide.h: follow_decide; csrc/mppi_costmap_rects.h:
// roll_bands, the one statement the host's rolls and the device's follows share): no device, no library.  Built like
// tools/costmap_rects_check.cpp, without contraction as the library is:
//   hipcc -x c++ -std=c++17 -O1 -ffp-contract=off  -Iccv_mppi_path_tracker_amd/csrc
//         tools/costmap_follow_check.cpp -o costmap_follow_check
//   ./costmap_follow_check decide < cases     one case per line: cx cy origin_x origin_y x y origin0_x origin0_y resolution nx ny margin
//                                             max_step (doubles as C99 hex floats or decimals); prints status dx dy cx' cy' origin_x'
//                                             origin_y' per case, the doubles as hex floats
//   ./costmap_follow_check bands N D R        every nx, ny <= N, |ex|, |ey| <= D, radius <= R: prints nx ny ex ey R n and the n
//                                             rectangles x0 y0 w h
// tests/test_follow_reference.py holds both outputs equal to tests/follow_reference.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mppi_costmap_follow_decide.h"
#include "mppi_costmap_rects.h"

using namespace ccv;

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "decide") == 0) {
        char line[1024];
        while (std::fgets(line, sizeof line, stdin)) {
            double v[13];
            char* at = line;
            int k = 0;
            for (; k < 13; ++k) {
                char* end = nullptr;
                v[k] = std::strtod(at, &end);
                if (end == at) break;
                at = end;
            }
            if (k != 13) return 2;
            const FollowFrame f{(int64_t)v[0], (int64_t)v[1], v[2], v[3]};
            const FollowDecision d = follow_decide(v[4], v[5], f, v[6], v[7], v[8], 1.0 / v[8], (int32_t)v[9], (int32_t)v[10], (int32_t)v[11], (int32_t)v[12]);
            std::printf("%d %d %d %lld %lld %a %a\n", d.status, d.dx, d.dy, (long long)d.frame.cx, (long long)d.frame.cy, d.frame.origin_x, d.frame.origin_y);
        }
        return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "bands") == 0) {
        const int N = std::atoi(argv[2]), D = std::atoi(argv[3]), Rmax = std::atoi(argv[4]);
        for (int nx = 1; nx <= N; ++nx)
            for (int ny = 1; ny <= N; ++ny)
                for (int ex = -D; ex <= D; ++ex)
                    for (int ey = -D; ey <= D; ++ey)
                        for (int R = 0; R <= Rmax; ++R) {
                            Rect band[kRollBands];
                            const int n = roll_bands(nx, ny, ex, ey, R, band);
                            std::printf("%d %d %d %d %d %d", nx, ny, ex, ey, R, n);
                            for (int k = 0; k < n; ++k) std::printf(" %d %d %d %d", band[k].x0, band[k].y0, band[k].w, band[k].h);
                            std::printf("\n");
                        }
        return 0;
    }
    return 2;
}

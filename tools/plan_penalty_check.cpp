// Stand-alone host run of what the weighted plan kernel quantises with (csrc/mppi_plan_penalty.h: plan_multiplier): no device, no
// library.  Built like tools/costmap_follow_check.cpp, without contraction as the library is:
//   hipcc -x c++ -std=c++17 -O1 -ffp-contract=off -Iccv_mppi_path_tracker_amd/csrc tools/plan_penalty_check.cpp -o plan_penalty_check
//   ./plan_penalty_check < cases      one case per line: cell gain max_penalty (the floats as C99 hex floats or decimals, nan and
//                                     inf included); prints m per case
// (add -fsanitize=address,undefined for a checked build: it is host code only)
// tests/test_plan_cost_reference.py holds the output equal to tests/plan_cost_reference.py.
#include <cstdio>
#include <cstdlib>

#include "mppi_plan_penalty.h"

int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char *at = line, *end = nullptr;
        const float cell = std::strtof(at, &end);
        if (end == at) return 2;
        at = end;
        const float gain = std::strtof(at, &end);
        if (end == at) return 2;
        at = end;
        const long max_penalty = std::strtol(at, &end, 10);
        if (end == at || max_penalty < 0 || max_penalty > ccv::kPlanMaxPenalty) return 2;
        std::printf("%u\n", ccv::plan_multiplier(cell, gain, (int32_t)max_penalty));
    }
    return 0;
}

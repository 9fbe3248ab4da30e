// Paths planned on the device (ccv_mppi_batch_resident_plan_enqueue): every named instance of a resident
// batch gets a new path from the cell its own resident pose lies in to a goal cell of its map, over the map's free cells.
// Integers only, but for one pose-to-cell step and one cell-to-pose step:
//     blocked(c) = !(cell(c) <= lethal)          (an fp32 compare: a NaN cell is blocked, a cell equal to lethal is free);
//                  everything outside the map is blocked
//     moves      (x, y) -> (x + dx, y + dy), dx, dy in {-1, 0, 1} not both zero; weight 5 straight, 7 diagonal; allowed iff the
//                target is not blocked and, for a diagonal, (x + dx, y) and (x, y + dy) are not blocked either (no corner is cut)
//     field      D uint16: kPlanBlocked on blocked cells, 0 on the goal, else min(kPlanFar, least total weight to the goal) -- the
//                one fixpoint of D(c) = min(D(c), min(kPlanFar, D(n) + w)), whatever the order of the relaxations
//     start      fx = (x - origin_x) * inv, fy likewise (the grid term's formula, no FMA); in = fx >= 0 && fx < nx && fy >= 0 &&
//                fy < ny; s = ((int)fx, (int)fy)
//     descent    from s, until D == 0: the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with D(n) + w == D(c)
//     pose i     the centre of cell i: origin_x + ((double)ix + 0.5) * resolution (one multiplication, one addition, no FMA)
// The kernel is k_plan.hip's; the entries live in the staging slot of the call (pinned host memory, read in place).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mppi_resident.h"

namespace ccv {

constexpr int kPlanMaxField = 81920;   // CCV_MPPI_PLAN_MAX_FIELD: (nx + 2)(ny + 2) at most
constexpr int kPlanMaxPoses = 16384;   // CCV_MPPI_PLAN_MAX_POSES (a descent has at most 65532 / 5 + 1 cells)
constexpr uint32_t kPlanBlocked = 65535u, kPlanFar = 65533u;
constexpr int kPlanResultInts = 6;     // a result row: status, poses, start cell x, y, D(start), sweeps

enum : int32_t { kPlanOk = 1, kPlanTruncated = 2, kPlanNoStart = 3, kPlanStartBlocked = 4, kPlanGoalBlocked = 5, kPlanUnreachable = 6,
                 kPlanNotConverged = 7 };

// One planning instance.  All writes to its path slice, its n_path, its result row and its field come from the one workgroup
// of its entry; the map is only read.
struct alignas(16) PlanEntry {
    const float* cells;     // [ny][nx] the map as the stream finds it
    const double* pose;     // the instance's resident pose: x, y
    double* path_x;         // [capacity] the instance's path slice ...
    double* path_y;         // ... and its y half
    BatchInstance* inst;    // the instance's row: n_path is written
    int32_t* result;        // [kPlanResultInts]
    uint16_t* field;        // [ny][nx] the field kept for the read-back, or null
    double origin_x, origin_y, inv, resolution;
    int32_t nx, ny, goal_x, goal_y;
    int32_t capacity, pad[3];
};
static_assert(sizeof(PlanEntry) == 128, "a table of the staging slot");

// One launch for the n entries of a call.
void launch_plan_field(const PlanEntry* entries, int32_t n, float lethal, int32_t max_sweeps, hipStream_t stream);

}  // namespace ccv

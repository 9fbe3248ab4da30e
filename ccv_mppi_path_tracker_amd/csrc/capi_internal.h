// Internal to the host side of the C ABI (include/ccv_mppi.h): the two handle types and the plumbing their units share.
//   ccv_mppi_capi.hip    life cycle, kernel-family rule and launch plan, the fused iteration and its update, result fetch
//   capi_exchange.hip    direct exchange of the partial vectors between the devices of a node
//   capi_resident.hip    device-resident closed loop of a single handle
//   capi_stage.hip       stage-wise calls, read-back, timing
//   capi_batch.hip       batch handles (ccv_mppi_batch_*): what a tick runs and what reads its results, the resident loop included
//   capi_batch_config.hip  batch handles: what configures the next launch (parameters, shifted weights, discs, fleet term)
//   capi_batch_maps.hip  batch handles: the maps of the grid term, a caller's cells or costmaps derived on the device, and the
//                        stream-ordered patches, rolls and scans of those
//   capi_batch_feed.hip  batch handles: best candidates and optimal paths of every instance (mppi_feed.h)
//   capi_batch_plan.hip  batch handles: paths planned on the device from the maps to goal cells (mppi_plan.h)
//   capi_batch_follow.hip  batch handles: costmaps that follow their robots, decided on the device (mppi_costmap_follow.h)
// A handle is made of named parts (below).  A part owns what it allocates, by type (capi_owned.h): device arrays, pinned staging
// and events go with the part, nothing is freed by a list; a raw pointer in a part is a view into an array declared beside it.  Core is what a single handle and a batch handle both have; the shared functions
// take the core, or the one part they work on where they need no more (those return the HIP error, the caller reports it).
// Everything here is C++ with internal names (namespace ccv): only the ccv_mppi_* entry points are extern "C".
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "capi_owned.h"
#include "fast_trig.h"
#include "mppi_kernels.h"
#include "mppi_launch.h"
#include "mppi_update.h"
#include "mppi_resident.h"
#include "mppi_fleet.h"

namespace ccv {

// K, H, R of one problem; pitch: the columns of the sample axis; nblocks: the workgroups of one problem's K
struct Shape {
    ccv_mppi_config cfg{};
    int udim = 0, K = 0, H = 0, R = 0, pitch = 0, nchunks = 0, nblocks = 0;
    int cu_count = 256;   // the device's CUs (set_shape): the kernel-family thresholds hang on it
};

// What select_kernels() decides at create; nothing assigns the families afterwards.  A launch's kernel: make_plan().
struct KernelChoice {
    KernelFamily stagewise = KernelFamily::FourWave;   // family of MODE_ROLLOUT / MODE_COST launches
    KernelFamily fused = KernelFamily::FourWave;       // family of the fused iteration: the same, or OneWave
    int lds_window = 1;                // CCV_MPPI_WINDOW=scalar -> 0: the plain kernel's scalar-load window variant (experiments)
    bool fast_clamp_allowed = true;    // clampd_fast (mppi_device_util.h) unless CCV_MPPI_FAST_CLAMP=0
    int prio_rotate = 0;               // pc_rotate_priority (mppi_handoff.h)
    int prune = 0;                     // pc_prune_window (mppi_consume.h)
};

struct DeviceBuffers {
    Stream own_stream;                 // (first: the stream outlives every array and event of the handle)
    hipStream_t stream = nullptr;      // own_stream, or the caller's (set_stream)
    DeviceArray<double> d_nominal;
    DeviceArray<char> d_arena;         // one allocation behind u, z, xs, ys, cost, w, partial (2 MB-aligned pieces)
    double* d_u = nullptr;             // a view into d_arena
    float* d_z = nullptr;              // a view into d_arena; the fused iteration stores the normals in place of the controls (mppi_kernels.h)
    DeviceArray<double> d_nom_used;    // ... and the warm start they were drawn around
    bool controls_in_z = false;        // d_u is stale: the controls of the last iteration are (d_z, d_nom_used)
    double* d_xs = nullptr;            // views into d_arena, these five
    double* d_ys = nullptr;
    double* d_cost = nullptr;
    double* d_w = nullptr;
    double* d_partial = nullptr;
    DeviceArray<double> d_statpart;
    DeviceArray<double> d_vec;
    DeviceArray<double> d_stats;
    DeviceArray<unsigned long long> d_dbg;   // -DCCV_DIAG builds only (mppi_diag.h): the kernels' stamp buffer
    DeviceArray<double> d_scratch;           // read-back staging (ensure_scratch)
    size_t scratch_bytes = 0;
    int nparts_last = 0;   // number of partial columns the last cost evaluation produced (fused: workgroups, else: chunks)
    double inj_absmax[CCV_MPPI_MAX_UDIM] = {0, 0, 0, 0, 0};   // largest |control| per dimension in the buffer (sampled: clamp bound)
    double nom_absmax[CCV_MPPI_MAX_UDIM] = {0, 0, 0, 0, 0};   // largest |u*| per dimension a caller has put there (track_absmax)
};

// result mailbox of the blocking calls (FinalizeArgs::mail): pinned host-mapped memory the update kernel writes; and the pinned
// host staging the result is decoded or copied into
struct Mailbox {
    PinnedArray<double> h_pin;
    size_t pin_doubles = 0;
    PinnedArray<unsigned long long> h_mail;
    unsigned long long* d_mail = nullptr;   // a view: h_mail as the device addresses it
    uint32_t mail_seq = 0;
    bool want_mail = false;      // the next plain update launch posts its result (set by the blocking entry points)
    bool mail_pending = false;   // ... and that launch is in flight: read_mail() polls the mailbox
    bool use_mail = true;        // CCV_MPPI_MAILBOX=0: copy + stream synchronisation instead (experiments)
};

// queue-depth throttle for the asynchronous entry points: beyond a few dozen iterations in flight the HIP runtime's
// enqueue path slows down several-fold (measured: 12 us/call at depth <= 64, 90 us/call at depth 512), so every
// kThrottleEvery-th enqueue records an event and waits for the one recorded kThrottleSlots marks earlier
struct Throttle {
    static constexpr int kThrottleEvery = 16, kThrottleSlots = 3;
    Event throttle_ev[kThrottleSlots];   // (its own rotation rule: the slot comes from the count)
    bool throttle_used[kThrottleSlots] = {false, false, false};
    uint64_t enqueued = 0;
    bool throttle = true;   // CCV_MPPI_THROTTLE=0 disables (experiments)
};

struct Timing {
    bool timing = false;
    int timing_every = 1;     // record events on every n-th iteration only
    int64_t timing_count = 0;
    std::vector<Event> ev;       // triples: rollout kernel begin, rollout kernel end, end of the launch sequence
    bool timed_now = false;      // the launch being enqueued is timed (timing_begin .. timing_end): its triple is
    size_t ev_slot = 0;          // ev[ev_slot .. ev_slot + 2]
    size_t ev_used = 0;
    double t_roll_sum = 0.0, t_iter_sum = 0.0;
    int64_t t_n = 0;
    float last_iter_us = 0.f, last_roll_us = 0.f;
};

// One update launch as a value (the update side's RolloutPlan): launch_finalize() and launch_finalize_advance() are the only
// places that turn it into a kernel.
struct UpdatePlan {
    FinalizeArgs args{};
    int batch = 0;                        // instances (the grid's y), 0: a single handle
    bool fused = true;                    // a batch's partial layout: the rollout kernels' (k_finalize_batch) or k_update_partials_batch's
    const BatchParams* shift = nullptr;   // a batch's shifted-weight update (the _shift kernels): its parameter table
    int K = 0;                            // ... and the instance's K
};

// device-resident loops: the update of a tick is launched together with the next tick's prologue (launch_finalize_advance);
// anything else that needs u*, the statistics or the stream first gets the plain update (flush_finalize)
struct DeferredUpdate {
    bool fin_pending = false;
    UpdatePlan fin{};
};

// (the order of the bases matters: DeviceBuffers, whose first member is the stream, comes before every base that holds an event
// or pinned memory, so the stream is destroyed after all of them)
struct Core : Shape, KernelChoice, DeviceBuffers, Mailbox, Throttle, Timing, DeferredUpdate {
    std::string err;
};

// ---- a single handle only ------------------------------------------------------------------------------------------------
struct StageState {
    bool have_controls = false, have_rollout = false, have_weights = false;
    double st_x0[5] = {0, 0, 0, 0, 0};
    double st_dt = 0.1;
    DeviceArray<double> d_cmin;   // CCV_MPPI_FLAG_MIN_SHIFT: the global minimum cost
};

// device-resident closed loop (mppi_resident.h)
struct ResidentLoop {
    DeviceArray<ResidentFrame> d_frame;
    DeviceArray<double> d_path;    // [2][n_path]: x then y
    DeviceArray<double> d_trace;   // [kTraceRows][6]
    static constexpr int kTraceRows = 8192;
    int n_path = 0;
    double path_resolution = 0.0;
    bool have_pose = false;
    int64_t res_steps = 0;                 // k_advance launches since the pose was set
    double res_angle_abs[3] = {0, 0, 0};   // conservative bounds on |yaw|, |roll|, |pitch| of the resident pose (fast_trig_safe)
};

// direct exchange of the partial vectors between the devices of a node (k_finalize_exchange, mppi_update.h)
struct Exchange {
    ExchangeBox* d_box = nullptr;                   // this device's box (peers write into it)
    ExchangeBox* box_peer[kMaxRanks] = {nullptr};   // every rank's box as mapped here ([xchg_rank] = d_box)
    bool box_opened[kMaxRanks] = {false};           // mapped with hipIpcOpenMemHandle (to be closed)
    double* d_xvec = nullptr;                       // reduced [sum w, sum w*u]
    int32_t* h_xflag = nullptr;                     // "a peer timed out" flag: pinned, host-mapped memory the update kernel writes
    int32_t* d_xflag = nullptr;                     // ... and its device address (sticky until the exchange is released)
    double xchg_timeout_s = 10.0;                   // (what the message says)
    int xchg_world = 0, xchg_rank = 0;
    bool xchg_connected = false;
    bool box_fine_grained = false;                  // the box is fine-grained (device-coherent) memory
    uint32_t xchg_nonce = 0;                        // this rank's contribution to the sequence base (rank 0's is used)
    uint32_t xchg_base = 0;                         // sequence numbers start here: a restarted job does not match old packets
    unsigned long long xchg_seq = 0;
    unsigned long long xchg_timeout_ticks = 1000000000ull;   // 10 s of the 100 MHz clock (CCV_MPPI_EXCHANGE_TIMEOUT_MS: tests)
};

}  // namespace ccv

using namespace ccv;

// (Core first: its stream outlives the arrays of the parts after it; Exchange is released by hand before the delete)
struct ccv_mppi_handle : Core, StageState, ResidentLoop, Exchange {
    // deferred division: u* = pending_vec[1..] / pending_vec[0] (ccv_mppi_apply_partials_enqueue, the exchange); the next fused
    // rollout divides while it stages the warm start, any other reader gets k_apply_partials first (flush_division)
    const double* pending_vec = nullptr;
};

// ---- a batch handle only (ccv_mppi_batch_*) -----------------------------------------------------------------------------
namespace ccv {

// the instances' records: per call, poses, dt, windows and noise keys go to the device as one block
struct BatchRecords {
    int rec_doubles = 0;
    DeviceArray<double> d_rec;                      // [B][rec_doubles]: BatchHead + window a[H], b[H], c[H] per instance
    static constexpr int kRecSlots = 4;             // pinned staging of the records: kRecSlots slots of B * rec_doubles doubles,
    StagingRing rec_ring;                           // not mapped -- the reader of a slot is batch_enqueue's hipMemcpyAsync
};

// device-resident closed loop of every instance (ccv_mppi_batch_resident_*, mppi_resident.h)
struct BatchResident {
    DeviceArray<ResidentFrame> d_rframe;    // [B]
    DeviceArray<BatchInstance> d_inst;      // [B]
    DeviceArray<double> d_rpath;            // [2][n_total]
    DeviceArray<double> d_rtrace;           // [B][CCV_MPPI_BATCH_TRACE_ROWS][6]
    int64_t n_total = 0;
    std::vector<BatchInstance> inst;        // host copy of d_inst
    std::vector<double> res_angle_abs;      // [B][3]: bounds on |yaw|, |roll|, |pitch| of every resident pose
    bool have_paths = false, have_poses = false;
    int64_t res_steps = 0;                  // resident ticks since the poses were set (every instance's step count)
};

// per-instance parameters (ccv_mppi_batch_set_params): the VARIED kernels read instance b's row of d_params through the
// pointer in its record's head; without them (varied = false) every instance has cfg and the shared kernels run.
// Shifted weights (ccv_mppi_batch_set_min_shift): the SHIFT rollout kernels and the _shift update kernels, always over the
// parameter table -- B copies of cfg in it while `varied` is false
struct ParamTable {
    bool varied = false;
    std::vector<ccv_mppi_config> cfgs;      // [B] the instances' configurations while varied
    DeviceArray<BatchParams> d_params;      // [B], allocated when a form from Varied up first needs it (sync_tables), kept until destroy
    bool min_shift = false;
    DeviceArray<double> d_cmin;             // [B]: the plain family's exact instance minima (k_min_cost_batch)
    bool shift_result = false;              // the last launch left block-relative weights in d_w (ccv_mppi_batch_read_weights)
};

// disc obstacles (ccv_mppi_batch_set_obstacles): the OBST rollout kernels, always over the parameter table too; the rows of
// the table point into d_obst.  Moving discs (ccv_mppi_batch_set_obstacle_velocities): the MOVING rollout kernels while
// `moving`; the rows of the table point into d_obst_v.  Every row of d_obst_v is defined from its allocation on: zero unless
// the caller gave a velocity (a neighbour's disc under fleet prediction: what the prologue wrote this tick).
struct Discs {
    bool obst = false;
    DeviceArray<double> d_obst;             // [B][CCV_MPPI_MAX_OBSTACLES][3], allocated at the first _set_obstacles, kept until destroy
    std::vector<double> obst_xyr;           // [B][CCV_MPPI_MAX_OBSTACLES][3] host copy while obst
    std::vector<int32_t> obst_n;            // [B]
    std::vector<double> obst_w;             // [B]
    bool moving = false;
    DeviceArray<double> d_obst_v;           // [B][CCV_MPPI_MAX_OBSTACLES][2], allocated when first needed (sync_tables), kept until destroy
    std::vector<double> obst_vxy;           // [B][CCV_MPPI_MAX_OBSTACLES][2] host copy while moving
};

// occupancy grids (ccv_mppi_batch_set_grids): the GRID rollout kernels while `grid`.  A grid plan is a moving plan: without
// discs the kernels see n_obst = 0 and read neither disc nor velocity rows; with discs and no velocities, d_obst_v is zero.
struct Grids {
    bool grid = false;
    DeviceArray<GridRow> d_grid_rows;       // [B], a row per instance (BatchParams::grid points at it, or is null)
    DeviceArray<float> d_grid_cells;        // the cells of all maps, one allocation
    std::vector<ccv_mppi_grid> grid_maps;   // host copy of the maps' geometry (cells: null)
    std::vector<size_t> grid_offset;        // [n_maps] first cell of map m in d_grid_cells
    std::vector<int32_t> grid_map_of;       // [B]
    std::vector<double> grid_w;             // [B]
};

// occupancy layers (ccv_mppi_batch_set_occupancy, mppi_costmap.h): while `occ`, the cells of Grids are not a caller's but derived
// on the device from a uint8 layer per map (same geometry, same offsets: layer m starts at d_occ + grid_offset[m]) and the map's
// inflation; patches of a layer, rolls of the maps' windows and range scans traced into the layers are enqueued on the stream
// (ccv_mppi_batch_update_ / _roll_ / _scan_occupancy_enqueue) through the staging ring (Staging, below).
struct Costmap {
    bool occ = false;
    DeviceArray<uint8_t> d_occ;              // the layers of all maps, one allocation
    DeviceArray<float> d_profile;            // the profile tables of all maps, one allocation
    // rolling maps (mppi_costmap_roll.h): a second allocation of the layers and of the float cells, same sizes and offsets, made at
    // the first roll and dropped with the layers.  A roll writes the one that does not hold the map and flips Layer::front.
    DeviceArray<uint8_t> d_occ_roll;
    DeviceArray<float> d_cells_roll;
    struct Layer {
        size_t profile_offset;               // first entry of the map's table in d_profile
        int32_t threshold, radius;           // radius: R, in cells
        float free_value;
        uint8_t front;                       // which allocation holds the map: 0 the first (d_occ, Grids::d_grid_cells), 1 the second
        int64_t cx, cy;                      // cells moved since _set_occupancy
        double ox0, oy0;                     // ... and the origin it was given
    };
    std::vector<Layer> layers;               // [n_maps]
    // the layers and tables go (the maps become a caller's, or none)
    void drop_layers() { *this = Costmap{}; }
};

// the staging ring of the *_enqueue calls: CCV_MPPI_OCC_PATCH_SLOTS mapped slots of CCV_MPPI_OCC_PATCH_MAX_CELLS bytes the kernels
// read in place.  Occupancy patches, rolls, scans, the world's patches, sensings and plans enqueue through it.  Made at the first
// _set_occupancy or _resident_set_plan (staging_create) and kept until destroy, whatever becomes of the layers, the world or the plan.
struct Staging {
    StagingRing ring;
};

// the simulated range sensor (ccv_mppi_batch_set_world / _resident_sense_enqueue, mppi_costmap_sense.h): one ground-truth occupancy
// map the resident robots' beams are cast through, the anchors that tie the occupancy layers' frames to it, and the read-back of
// the last sensing per instance.  Lives from _set_world to _set_world(NULL), the next _set_occupancy or _set_grids (the anchors
// speak of those layers) or destroy.
struct InflateArgs;
struct World {
    bool world = false;
    ccv_mppi_occupancy world_geo = {};       // the world's geometry and threshold (cells: null)
    DeviceArray<uint8_t> d_world;            // [ny][nx]
    DeviceArray<int32_t> d_sense_first;      // [B][world_max_beams]: the blocked cell of every beam, -1 without
    DeviceArray<int32_t> d_sense_cell;       // [B][2]: the robots' world cells, (-1, -1) for one that sensed nothing
    DeviceArray<InflateArgs> d_sense_rects;  // [B]: the rectangles k_sense_trace writes and k_inflate_rects reads
    std::vector<int32_t> world_anchor;       // [n_maps][2]: the world cell of the map's cell (0, 0) at _set_occupancy
    int32_t world_max_beams = 0;
    void drop_world() { *this = World{}; }
};

// paths planned on the device (ccv_mppi_batch_resident_set_plan / _plan_enqueue, mppi_plan.h; capi_batch_plan.hip): while `plan`,
// BatchResident::d_rpath has room for max(n_path, capacity) poses per instance and the device's BatchInstance::n_path is the
// truth -- the host copy's n_path is what the last setter saw.  Lives from _set_plan to _set_plan(NULL), the next
// _resident_set_paths or destroy.
struct Plan {
    bool plan = false, plan_keep = false;
    std::vector<int32_t> plan_capacity;      // [B] poses a plan may write, 0: the instance does not plan
    std::vector<int32_t> plan_field_of;      // [B] the instance's field in d_plan_fields, -1 without
    std::vector<int32_t> plan_dims;          // [B][2]: nx, ny of the map of the instance's last plan call
    DeviceArray<int32_t> d_plan_result;      // [B][6]: status, poses, start cell, D(start), sweeps of every instance's last plan
    DeviceArray<uint16_t> d_plan_fields;     // [instances with capacity][CCV_MPPI_PLAN_MAX_FIELD], with keep_fields
    // traversal weights (_resident_set_plan_penalty, mppi_plan_cost.h): host state only; (0, 0) after every _set_plan
    float plan_gain = 0.0f;
    int32_t plan_max_penalty = 0;
    void drop_plan() { *this = Plan{}; }
};

// costmaps that follow their robots (ccv_mppi_batch_resident_set_follow / _follow_enqueue, mppi_costmap_follow.h): while `follow`
// the device's frame table is the truth of every map's rolled offset and origin -- Costmap::Layer::cx, cy and the origins of
// Grids::grid_maps are what the last call that synchronised saw (follow_refresh) -- and Layer::front stays the host's: a named
// map changes buffers at every call.  Lives from _set_follow(1) to _set_follow(0), the next _set_occupancy or _set_grids or destroy.
struct FollowFrame;
struct SenseEntry;
struct PlanEntry;
struct Follow {
    bool follow = false;
    DeviceArray<FollowFrame> d_follow_frames;   // [n_maps][2]: the slot follow_slot[m] is map m's current frame
    DeviceArray<int32_t> d_follow_result;       // [n_maps][4]: status, dx, dy, 0 of every map's last call
    DeviceArray<InflateArgs> d_follow_rects;    // [n_maps][4]: the bands k_follow_shift writes and k_inflate_rects reads
    DeviceArray<SenseEntry> d_follow_sense;     // [B]: a sensing's entries, completed on the device
    DeviceArray<PlanEntry> d_follow_plan;       // [B]: a plan's
    std::vector<uint8_t> follow_slot;           // [n_maps]: the parity of the map's follow count
    void drop_follow() { *this = Follow{}; }
};

// fleet term (ccv_mppi_batch_resident_set_fleet, mppi_fleet.h): the resident prologue appends discs for the nearest other
// robots to every instance's list.  While it is on the obstacle kernels run whether or not `obst` is set, over d_obst and
// the three obst_* vectors (obst_n: the static counts, all 0 without static discs; obst_w: the one weight per instance).
// Fleet prediction (ccv_mppi_batch_set_fleet_prediction): the velocities travel with the positions, a neighbour's disc moves
// with the velocity its robot had over the last tick, and the MOVING kernels run (over d_obst_v: the static rows the host's,
// zero without ccv_mppi_batch_set_obstacle_velocities; the fleet's rows written by the prologue every tick)
struct Fleet {
    bool fleet = false;
    DeviceArray<double> d_fleet_xy;         // [2][B][2]: tick n reads half n & 1 and writes the other (n = res_steps)
    DeviceArray<double> d_fleet_radius;     // [B]
    DeviceArray<int32_t> d_fleet_nstatic;   // [B]: obst_n on the device, for the prologue (sync_tables)
    std::vector<double> fleet_radius;       // [B]
    double fleet_range = 0.0;
    int32_t fleet_maxn = 0;
    bool fleet_pred = false;
    DeviceArray<double> d_fleet_v;          // [2][B][2]: tick n reads half n & 1 and writes the other, like d_fleet_xy
};

}  // namespace ccv

// One configuration, B instances on one sample axis of B * Kpad columns (Kpad = K rounded up to 64; mppi_kernels.h,
// batch_view): the core of a single handle, whose K is the instance's and whose
// pitch is the batch's.  Per call, the instances' poses, dt, windows and noise keys go to the device as one block of records;
// one rollout launch, one update launch (k_finalize_batch), one mailbox of B * (R + 4) slots under one sequence number.
// (Core first: its stream outlives the arrays, rings and events of the parts after it)
struct ccv_mppi_batch : Core, BatchRecords, BatchResident, ParamTable, Discs, Grids, Costmap, Staging, World, Plan, Follow, Fleet {
    int B = 0, kpad = 0;
    int last_kernel = -1;   // CCV_MPPI_BATCH_KERNEL_* of the last launch, -1 before the first
    bool mail_any_size = false;   // CCV_MPPI_BATCH_MAIL=1: the mailbox however many slots (measurement)
    bool have_result = false;
};

namespace ccv {

inline int fail(Core* h, int code, const char* what, hipError_t e = hipSuccess) {
    if (h) {
        h->err = what;
        if (e != hipSuccess) {
            h->err += ": ";
            h->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIP_TRY(h, call)                                                            \
    do {                                                                            \
        hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) return fail((h), CCV_MPPI_ERR_HIP, #call, e__);      \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The caller's current device is put back when an entry point that had to switch to the handle's device returns (on error
// paths too): a process that drives several devices must not find its current device changed behind its back.
struct DeviceGuard {
    int prev = -1, mine = -1;
    explicit DeviceGuard(int device) : mine(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != mine) (void)hipSetDevice(prev);
    }
};

// ---- life cycle (ccv_mppi_capi.hip) -------------------------------------------------------------------------------------
int check_config(const ccv_mppi_config* cfg);   // abi_version, model, num_samples, horizon: before a device is looked at
int check_device(int device);                   // CCV_MPPI_ERR_NO_DEVICE unless `device` exists
void set_shape(Shape& s, const ccv_mppi_config& cfg, int pitch, int nblocks);
void select_kernels(KernelChoice& k, const Shape& s, int64_t workgroups, bool batched);
// element counts of the device and pinned buffers whose size differs between a single handle and a batch
struct BufferCounts {
    size_t nparts_max;   // partial columns (workgroups or chunks, whichever is more)
    size_t nominal, vec, stats;
    DeviceArray<double>* extra;   // one more zeroed array of doubles: d_cmin of a single handle, d_rec of a batch
    size_t n_extra;
    size_t pin_doubles, mail_slots;
};
int create_buffers(Core* h, const BufferCounts& n);
void wait_for_streams(Core* h);   // before a handle is deleted: its stream and, under a caller's stream, its own are idle
int set_stream(Core* h, void* hip_stream);
hipError_t ensure_scratch(DeviceBuffers& d, size_t bytes);

// ---- the launch plan (ccv_mppi_capi.hip) --------------------------------------------------------------------------------
enum : int { kTrigUnsafe = 0, kTrigSafe = 1, kTrigWide = 2 };
// has_wide: the launch's family has a wide-turn form (has_wide_form)
int fast_trig_safe(const Core* h, const ccv_mppi_config& c, const RolloutArgs& A, int mode, bool has_wide);
inline KernelFamily family_of(const KernelChoice& k, const int mode) { return mode == MODE_FUSED ? k.fused : k.stagewise; }
inline bool has_wide_form(const KernelChoice& k, const int mode) {
    return mode == MODE_FUSED && (k.fused == KernelFamily::FourWave || k.fused == KernelFamily::OneWave);
}
// The kernel of one launch: the family chosen at create, demoted to the plain kernel when the headings are unbounded
// (trig = fast_trig_safe of the launch; a batch: of its worst instance), the wide-turn form when trig says so.
// form: what the launch serves (BatchForm, mppi_kernels.h; a batch handle's: batch_form(), capi_batch_config.hip); shift (a batch in
// shifted-weight mode): with a form from Varied up.
inline RolloutPlan make_plan(const KernelChoice& k, const int model, const int mode, const int trig, const int batch, const BatchForm form,
                             const bool shift) {
    KernelFamily f = trig == kTrigUnsafe ? KernelFamily::Plain : family_of(k, mode);
    // (the four-wave kernel runs a plan whose form the one-wave kernel lacks, at any number of workgroups)
    if (f == KernelFamily::OneWave && !has_one_wave_form(model, form)) f = KernelFamily::FourWave;
    return RolloutPlan{f, model, mode, f != KernelFamily::Plain && trig == kTrigWide, batch, form, shift, k.lds_window != 0};
}

RolloutPlan plan_of(const ccv_mppi_handle* h, const RolloutArgs& A, int mode);   // a single handle's

// ---- the fused iteration and its update (ccv_mppi_capi.hip) -------------------------------------------------------------
void fill_params(const ccv_mppi_config& c, bool fast_clamp_allowed, RolloutArgs& A);
void fill_args(const Core* h, RolloutArgs& A, const double* x0, double dt, double yaw_ref0, uint64_t seed, uint64_t iter);
void window_coeffs(int H, const double* x_ref, const double* y_ref, double px, double py, double* a, double* b, double* c);
void track_absmax(const double* u, size_t n, int udim, double* absmax);
// the update kernel of a plan: k_finalize, k_finalize_batch or k_finalize_batch_shift
void launch_finalize(Core& h, const UpdatePlan& p);
// ... together with the next tick's prologue: k_finalize_advance (V), or k_finalize_advance_batch / _varied / _shift (G; table:
// the per-instance parameters the prologue reads, or null).
void launch_finalize_advance(Core& h, const UpdatePlan& p, const AdvanceArgs& V);
// fleet: the fleet forms of the _varied / _shift kernels (mppi_fleet.h; they write the table's n_obst), or null; pred (with
// fleet): their prediction forms (k_fleet_pred.hip), or null
void launch_finalize_advance(Core& h, const UpdatePlan& p, const BatchAdvanceArgs& G, BatchParams* table, const FleetArgs* fleet = nullptr,
                             const FleetPredArgs* pred = nullptr);
int flush_finalize(Core* h);                // the deferred update now (launch_finalize)
int flush_division(ccv_mppi_handle* h);     // the deferred division now: k_apply_partials
int flush_pending(ccv_mppi_handle* h);      // both, in that order
int materialize_controls(ccv_mppi_handle* h);
int launch_rollout(ccv_mppi_handle* h, const RolloutArgs& A, const Window& W, int mode);
int launch_sample(ccv_mppi_handle* h, const RolloutArgs& A);
UpdateArgs update_args(const Core* h);
FinalizeArgs finalize_args(const Core* h, double* vec, int nparts, bool normalise);
void post_to_mail(Mailbox& m, FinalizeArgs& F);
int launch_update(ccv_mppi_handle* h, bool normalise, double* vec_out, bool exchange = false, bool defer = false);
int check_iter_args(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref);
int enqueue_iteration(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref, double yaw_ref0,
                      uint64_t seed, uint64_t iter, bool normalise, double* vec_out, bool resident = false, bool exchange = false);
hipError_t throttle_tick(Throttle& t, hipStream_t stream);
// a timed launch: begin .. rollout kernel (its LaunchAt from timing_rollout_at, then timing_rollout_done) .. update .. end
hipError_t timing_begin(Timing& t);
hipError_t timing_rollout_at(const Timing& t, hipStream_t stream, bool plain, LaunchAt& at);
hipError_t timing_rollout_done(const Timing& t, hipStream_t stream, bool plain);
hipError_t timing_end(Timing& t, hipStream_t stream);
hipError_t timing_collect(Timing& t, hipStream_t stream);
int timing_enable(Core* h, int32_t on);   // ccv_mppi_timing_enable / _read and their batch forms (capi_stage.hip)
int timing_read(Core* h, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters, int32_t reset);
int read_mail(Core* h, size_t n_slots, double* out);
void unpack_result(const Timing& t, int R, const double* v, double* u_opt_out, ccv_mppi_stats* stats);
int fetch_result(ccv_mppi_handle* h, double* u_opt_out, ccv_mppi_stats* stats);

// ---- direct exchange (capi_exchange.hip) --------------------------------------------------------------------------------
void exchange_release(ccv_mppi_handle* h);
int exchange_check(ccv_mppi_handle* h);

// ---- device-resident loop (capi_resident.hip) ---------------------------------------------------------------------------
// pose and step counter: the head of a ResidentFrame, as the host writes it
struct FrameHead {
    double x0[5];
    double yaw_ref0;
    int32_t index, steps;
};
static_assert(offsetof(ResidentFrame, W) == sizeof(FrameHead), "frame head layout");
struct ResidentBounds {
    double angle[3];   // bounds on |yaw|, |roll|, |pitch| after this tick
    double heading;    // bound on the heading the prologue itself takes sin / cos of
};
ResidentBounds resident_bounds(const DeviceBuffers& d, const ccv_mppi_config& c, const double* angle_abs, double dt, int32_t advance);
hipError_t read_trace_ring(const double* d_ring, int64_t cap, int64_t steps, int32_t max_rows, double* rows, int32_t* n_rows);

// ---- batch handles: what the tick path (capi_batch.hip) and the setters (capi_batch_config.hip, capi_batch_maps.hip) share ---
// instance b's configuration: its own under per-instance parameters, the creation configuration otherwise
inline const ccv_mppi_config& batch_cfg(const ccv_mppi_batch* bh, const int b) { return bh->varied ? bh->cfgs[(size_t)b] : bh->cfg; }
// the rung of the kernels the handle's next launch runs (BatchForm, mppi_kernels.h): the highest one whose addition is on
BatchForm batch_form(const ccv_mppi_batch* bh);
// whether the kernels read the parameter table
inline bool uses_table(const ccv_mppi_batch* bh) { return batch_form(bh) >= BatchForm::Varied; }
// a deferred resident update (batch_launch) is launched now
inline int batch_flush(ccv_mppi_batch* bh) { return flush_finalize(bh); }
// the handle's device current, no update deferred, the stream idle: nothing queued reads a table or writes a result any more
int quiesce(ccv_mppi_batch* bh);
// the derived tables the next launch or prologue reads, from the handle's state (capi_batch_config.hip); the caller has quiesced
int sync_tables(ccv_mppi_batch* bh);
inline bool valid_weight(const double w) { return w >= 0.0 && std::isfinite(w); }
// the fleet's snapshots start over (the caller has quiesced): both halves of the position table from xy [B][2] (null: as they are)
// and, under prediction, both halves of the velocity snapshot zero -- no robot has moved yet
int fleet_restart(ccv_mppi_batch* bh, const double* xy);

// ---- batch handles: the staging ring of the *_enqueue calls (Staging; StagingRing: capi_owned.h), for the units that enqueue through it ---
inline hipError_t staging_create(ccv_mppi_batch* bh) {   // at the first _set_occupancy or _resident_set_plan; idempotent
    return bh->ring.create(CCV_MPPI_OCC_PATCH_SLOTS, CCV_MPPI_OCC_PATCH_MAX_CELLS, /*mapped=*/true);
}
// the float cells that hold map m now: the second allocation after an odd number of rolls (Costmap::Layer::front)
float* cells_of(const ccv_mppi_batch* bh, int m, bool back = false);
// ... and the layer
uint8_t* layer_of(const ccv_mppi_batch* bh, int m, bool back = false);
// the second set of layers and float cells (Costmap::d_occ_roll, d_cells_roll), made once: quiesces like a setter if it allocates
int ensure_roll_buffers(ccv_mppi_batch* bh);
// while the maps follow (Follow): the stream idle and the host's copies of every map's offset and origin as the device has them
int follow_refresh(ccv_mppi_batch* bh);

}  // namespace ccv

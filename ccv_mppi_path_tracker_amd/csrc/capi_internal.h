// Internal to the host side of the C ABI (include/ccv_mppi.h): the two handle types and the plumbing their units share.
//   ccv_mppi_capi.hip    life cycle, kernel selection, the fused iteration and its update, result fetch
//   capi_exchange.hip    direct exchange of the partial vectors between the devices of a node
//   capi_resident.hip    device-resident closed loop of a single handle
//   capi_stage.hip       stage-wise calls, read-back, timing
//   capi_batch.hip       batch handles (ccv_mppi_batch_*), their resident loop included
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

#include "fast_trig.h"
#include "mppi_kernels.h"
#include "mppi_launch.h"
#include "mppi_update.h"
#include "mppi_resident.h"

using namespace ccv;

struct ccv_mppi_handle {
    ccv_mppi_config cfg{};
    int udim = 0, K = 0, H = 0, R = 0, pitch = 0, nchunks = 0, nblocks = 0;
    int nparts_last = 0;   // number of partial columns the last cost evaluation produced (fused: workgroups, else: chunks)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // device buffers
    double* d_nominal = nullptr;
    const double* pending_vec = nullptr;   // deferred apply_partials: u* = pending_vec[1..] / pending_vec[0] (see flush_pending)
    // device-resident loop: the update of a tick is launched together with the next tick's prologue (k_finalize_advance);
    // anything else that needs u* / the statistics first gets a plain k_finalize (flush_pending)
    bool fin_pending = false;
    FinalizeArgs fin_args{};
    double* d_u = nullptr;
    void* d_arena = nullptr;           // one allocation behind u, z, xs, ys, cost, w, partial (2 MB-aligned pieces)
    float* d_z = nullptr;              // the fused iteration stores the normals in place of the controls (mppi_kernels.h)
    double* d_nom_used = nullptr;      // ... and the warm start they were drawn around
    bool controls_in_z = false;        // d_u is stale: the controls of the last iteration are (d_z, d_nom_used)
    double* d_xs = nullptr;
    double* d_ys = nullptr;
    double* d_cost = nullptr;
    double* d_w = nullptr;
    double* d_partial = nullptr;
    double* d_statpart = nullptr;
    double* d_vec = nullptr;
    double* d_stats = nullptr;
    double* d_cmin = nullptr;
    unsigned long long* d_dbg = nullptr;   // -DCCV_DIAG builds only (mppi_diag.h): the kernels' stamp buffer
    // device-resident closed loop (mppi_resident.h)
    ResidentFrame* d_frame = nullptr;
    double* d_path = nullptr;    // [2][n_path]: x then y
    double* d_trace = nullptr;   // [kTraceRows][6]
    static constexpr int kTraceRows = 8192;
    int n_path = 0;
    double path_resolution = 0.0;
    bool have_pose = false;
    int64_t res_steps = 0;                 // k_advance launches since the pose was set
    double res_angle_abs[3] = {0, 0, 0};   // conservative bounds on |yaw|, |roll|, |pitch| of the resident pose (fast_trig_safe)
    // direct exchange of the partial vectors between the devices of a node (k_finalize_exchange, mppi_kernels.h)
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
    // queue-depth throttle for the asynchronous entry points: beyond a few dozen iterations in flight the HIP runtime's
    // enqueue path slows down several-fold (measured: 12 us/call at depth <= 64, 90 us/call at depth 512), so every
    // kThrottleEvery-th enqueue records an event and waits for the one recorded kThrottleSlots marks earlier
    static constexpr int kThrottleEvery = 16, kThrottleSlots = 3;
    hipEvent_t throttle_ev[kThrottleSlots] = {nullptr, nullptr, nullptr};
    bool throttle_used[kThrottleSlots] = {false, false, false};
    uint64_t enqueued = 0;
    bool throttle = true;   // CCV_MPPI_THROTTLE=0 disables (experiments)
    double* d_scratch = nullptr;  // read-back staging
    size_t scratch_bytes = 0;
    // pinned host staging
    double* h_pin = nullptr;
    size_t pin_doubles = 0;
    // result mailbox of the blocking calls (FinalizeArgs::mail): pinned host-mapped memory the update kernel writes
    unsigned long long* h_mail = nullptr;
    unsigned long long* d_mail = nullptr;   // its device address
    uint32_t mail_seq = 0;
    bool want_mail = false;      // the next plain k_finalize launch posts its result (set by the blocking entry points)
    bool mail_pending = false;   // ... and that launch is in flight: fetch_result() polls the mailbox
    bool use_mail = true;        // CCV_MPPI_MAILBOX=0: copy + stream synchronisation instead (experiments)
    // stage-wise state
    bool have_controls = false, have_rollout = false, have_weights = false;
    double st_x0[5] = {0, 0, 0, 0, 0};
    double st_dt = 0.1;
    // kernel selection (experiments): CCV_MPPI_KERNEL=v1 -> one-sample-per-lane k_rollout_cost,
    // CCV_MPPI_WINDOW=scalar -> its scalar-load window variant; default = k_rollout_pc
    int lds_window = 1;
    int coop = 1;
    bool solo = false;   // fused iterations run k_rollout_solo (one wave per 64 samples) instead of coop's kernel
    bool wide_turn = false;   // this launch: diff drive beyond |w|max dt = pi/4 -> the full-range sin / cos instantiation
    bool fast_clamp_allowed = true;   // clampd_fast (mppi_kernels.h) unless CCV_MPPI_FAST_CLAMP=0
    int prio_rotate = 0, cu_count = 256;   // pc_rotate_priority (mppi_rollout_pc.h)
    int prune = 0;                         // pc_prune_window (mppi_rollout_pc.h)
    double inj_absmax[CCV_MPPI_MAX_UDIM] = {0, 0, 0, 0, 0};   // largest |control| per dimension in the buffer (sampled: clamp bound)
    double nom_absmax[CCV_MPPI_MAX_UDIM] = {0, 0, 0, 0, 0};   // largest |u*| per dimension a caller has put there (ccv_mppi_set_nominal)
    // timing
    bool timing = false;
    int timing_every = 1;     // record events on every n-th iteration only
    int64_t timing_count = 0;
    std::vector<hipEvent_t> ev;  // triples: rollout kernel begin, rollout kernel end, end of the launch sequence
    bool timed_now = false;      // the launch being enqueued is timed (timing_begin .. timing_end): its triple is
    size_t ev_slot = 0;          // ev[ev_slot .. ev_slot + 2]
    size_t ev_used = 0;
    double t_roll_sum = 0.0, t_iter_sum = 0.0;
    int64_t t_n = 0;
    float last_iter_us = 0.f, last_roll_us = 0.f;
    std::string err;
};

// One configuration, B instances on one sample axis of B * Kpad columns (Kpad = K rounded up to 64; mppi_kernels.h,
// batch_view): the buffers, the stream, the mailbox and the timing of a ccv_mppi_handle whose K is the instance's and whose
// pitch is the batch's.  Per call, the instances' poses, dt, windows and noise keys go to the device as one block of records;
// one rollout launch, one update launch (k_finalize_batch), one mailbox of B * (R + 4) slots under one sequence number.
struct ccv_mppi_batch {
    ccv_mppi_handle h;
    int B = 0, kpad = 0, rec_doubles = 0;
    double* d_rec = nullptr;                        // [B][rec_doubles]: BatchHead + window a[H], b[H], c[H] per instance
    static constexpr int kRecSlots = 4;             // pinned staging of the records, in rotation: a slot is refilled only
    double* h_rec[kRecSlots] = {nullptr, nullptr, nullptr, nullptr};   // after the copy that read it has run
    hipEvent_t rec_ev[kRecSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool rec_used[kRecSlots] = {false, false, false, false};
    int rec_next = 0;
    int last_kernel = -1;   // CCV_MPPI_BATCH_KERNEL_* of the last launch, -1 before the first
    bool mail_any_size = false;   // CCV_MPPI_BATCH_MAIL=1: the mailbox however many slots (measurement)
    bool have_result = false;
    // device-resident closed loop of every instance (ccv_mppi_batch_resident_*, mppi_resident.h): the update of a resident
    // tick is launched together with the next tick's prologue (k_finalize_advance_batch); anything else that needs u*, the
    // statistics or the stream first gets a plain k_finalize_batch (batch_flush)
    bool fin_pending = false;
    FinalizeArgs fin_args{};
    ResidentFrame* d_rframe = nullptr;      // [B]
    BatchInstance* d_inst = nullptr;        // [B]
    double* d_rpath = nullptr;              // [2][n_total]
    double* d_rtrace = nullptr;             // [B][CCV_MPPI_BATCH_TRACE_ROWS][6]
    int64_t n_total = 0;
    std::vector<BatchInstance> inst;        // host copy of d_inst
    std::vector<double> res_angle_abs;      // [B][3]: bounds on |yaw|, |roll|, |pitch| of every resident pose
    bool have_paths = false, have_poses = false;
    int64_t res_steps = 0;                  // resident ticks since the poses were set (every instance's step count)
    // per-instance parameters (ccv_mppi_batch_set_params): the VARIED kernels read instance b's row of d_params through the
    // pointer in its record's head; without them (varied = false) every instance has h.cfg and the shared kernels run
    bool varied = false;
    std::vector<ccv_mppi_config> cfgs;      // [B] the instances' configurations while varied
    BatchParams* d_params = nullptr;        // [B], allocated at the first _set_params, freed at destroy
};

namespace ccv {

inline int fail(ccv_mppi_handle* h, int code, const char* what, hipError_t e = hipSuccess) {
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
void set_shape(ccv_mppi_handle* h, const ccv_mppi_config& cfg, int pitch, int nblocks);
void select_kernels(ccv_mppi_handle* h, int64_t workgroups, bool batched);
// element counts of the device and pinned buffers whose size differs between a single handle and a batch
struct BufferCounts {
    size_t nparts_max;   // partial columns (workgroups or chunks, whichever is more)
    size_t nominal, vec, stats;
    double** extra;      // one more zeroed array of doubles: d_cmin of a single handle, d_rec of a batch
    size_t n_extra;
    size_t pin_doubles, mail_slots;
};
int create_buffers(ccv_mppi_handle* h, const BufferCounts& n);
void release_buffers(ccv_mppi_handle* h);
int set_stream(ccv_mppi_handle* h, void* hip_stream);
int ensure_scratch(ccv_mppi_handle* h, size_t bytes);

// ---- the fused iteration and its update (ccv_mppi_capi.hip) -------------------------------------------------------------
void fill_params(const ccv_mppi_config& c, bool fast_clamp_allowed, RolloutArgs& A);
void fill_args(const ccv_mppi_handle* h, RolloutArgs& A, const double* x0, double dt, double yaw_ref0, uint64_t seed, uint64_t iter);
void window_coeffs(int H, const double* x_ref, const double* y_ref, double px, double py, double* a, double* b, double* c);
enum : int { kTrigUnsafe = 0, kTrigSafe = 1, kTrigWide = 2 };
int fast_trig_safe(const ccv_mppi_handle* h, const ccv_mppi_config& c, const RolloutArgs& A, int mode);
int fast_trig_safe(const ccv_mppi_handle* h, const RolloutArgs& A, int mode);
int flush_pending(ccv_mppi_handle* h);
int materialize_controls(ccv_mppi_handle* h);
int launch_rollout(ccv_mppi_handle* h, const RolloutArgs& A, const Window& W, int mode);
int launch_sample(ccv_mppi_handle* h, const RolloutArgs& A);
UpdateArgs update_args(const ccv_mppi_handle* h);
FinalizeArgs finalize_args(const ccv_mppi_handle* h, double* vec, int nparts, bool normalise);
void post_to_mail(ccv_mppi_handle* h, FinalizeArgs& F);
int launch_update(ccv_mppi_handle* h, bool normalise, double* vec_out, bool exchange = false, bool defer = false);
int check_iter_args(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref);
int enqueue_iteration(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref, double yaw_ref0,
                      uint64_t seed, uint64_t iter, bool normalise, double* vec_out, bool resident = false, bool exchange = false);
int throttle_tick(ccv_mppi_handle* h);
// a timed launch: begin .. rollout kernel (its LaunchAt from timing_rollout_at, then timing_rollout_done) .. update .. end
int timing_begin(ccv_mppi_handle* h);
int timing_rollout_at(ccv_mppi_handle* h, bool plain, LaunchAt& at);
int timing_rollout_done(ccv_mppi_handle* h, bool plain);
int timing_end(ccv_mppi_handle* h);
int timing_collect(ccv_mppi_handle* h);
int wait_mail(ccv_mppi_handle* h, size_t n_slots);
void decode_mail(const ccv_mppi_handle* h, size_t n_slots, double* out);
void unpack_result(const ccv_mppi_handle* h, const double* v, double* u_opt_out, ccv_mppi_stats* stats);
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
ResidentBounds resident_bounds(const ccv_mppi_handle* h, const ccv_mppi_config& c, const double* angle_abs, double dt, int32_t advance);
int read_trace_ring(ccv_mppi_handle* h, const double* d_ring, int64_t cap, int64_t steps, int32_t max_rows, double* rows, int32_t* n_rows);

}  // namespace ccv

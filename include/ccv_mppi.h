/*
 * ccv_mppi.h -- C ABI of the MI355X-native MPPI hot path (libccv_mppi_hip.so).
 *
 * Drop-in boundary for the four hot methods of the reference controller classes of
 * YoshikiMaekawa2000/ccv_mppi_path_tracker.  The reference has no FFI/plugin interface
 * (SURVEY.md 8b): the seam is the bodies of the private methods
 *
 *     sampling()                    src/diff_drive_mppi.cpp:81-102   src/steering_diff_drive_mppi.cpp:97-118   src/full_body_mppi.cpp:491-520
 *     predict_States()              src/diff_drive_mppi.cpp:111-124  src/steering_diff_drive_mppi.cpp:127-140  src/full_body_mppi.cpp:454-489
 *     calc_Weights()                src/diff_drive_mppi.cpp:212-223  src/steering_diff_drive_mppi.cpp:228-239  src/full_body_mppi.cpp:426-443
 *     determine_OptimalSolution()   src/diff_drive_mppi.cpp:225-246  src/steering_diff_drive_mppi.cpp:241-264  src/full_body_mppi.cpp:308-333
 *
 * called once each, in this order, from run() (src/diff_drive_mppi.cpp:352-358).  INTEGRATION.md
 * shows the patch a maintainer applies to those method bodies.
 *
 * Conventions (mirroring the reference):
 *   - plain C, no exceptions; every function returns an int status (0 = OK, <0 = error) and never aborts;
 *   - an opaque handle owns all device memory, allocated once in ccv_mppi_create() (the reference allocates
 *     everything once in the constructor, src/diff_drive_mppi.cpp:36-46) and never resized;
 *   - the caller owns all host arrays; pointers are host pointers unless a parameter name starts with `dev_`;
 *   - one handle = one caller thread; a call that hands data back to the host (ccv_mppi_iterate, ccv_mppi_update, the
 *     read-backs, ccv_mppi_get_nominal) returns when that data is complete; calls named *_enqueue and the stage-wise calls
 *     that return nothing to the host (ccv_mppi_sample, ccv_mppi_rollout, ccv_mppi_weights -- void methods in the
 *     reference) only enqueue work on the handle's stream, which keeps the order; ccv_mppi_synchronize waits for all of it;
 *   - all floating point data is IEEE double (the reference computes in double throughout);
 *   - there is NO CPU fallback: without a usable HIP device every call fails with CCV_MPPI_ERR_NO_DEVICE.
 */
#ifndef CCV_MPPI_H_
#define CCV_MPPI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCV_MPPI_ABI_VERSION 1
#define CCV_MPPI_MAX_UDIM 5
#define CCV_MPPI_MAX_HORIZON 128 /* window coefficients travel in the kernel-argument segment */

/* status codes */
#define CCV_MPPI_OK 0
#define CCV_MPPI_ERR_INVALID_ARG (-1)
#define CCV_MPPI_ERR_NO_DEVICE (-2)
#define CCV_MPPI_ERR_HIP (-3)
#define CCV_MPPI_ERR_STATE (-4) /* stage-wise calls in the wrong order */
#define CCV_MPPI_ERR_ALLOC (-5)
#define CCV_MPPI_ERR_TIMEOUT (-6) /* direct exchange: a peer's partial vector never arrived (reported at the next synchronisation) */

/* controller model; u_dim = 2 / 3 / 5, control order = declaration order of the reference
 * (dd: v,w  sd: v,w,steer  fb: v,w,direction,roll_v,pitch_v) */
#define CCV_MPPI_DIFF_DRIVE 0
#define CCV_MPPI_STEERING_DIFF_DRIVE 1
#define CCV_MPPI_FULL_BODY 2

/* flags */
#define CCV_MPPI_FLAG_ROLL_OFF 0x1   /* src/full_body_mppi.cpp:43-46: zmp_weight = roll_v_weight = 0 */
#define CCV_MPPI_FLAG_STEER_OFF 0x2  /* src/full_body_mppi.cpp:517: direction forced to 0 after the draw */
#define CCV_MPPI_FLAG_MIN_SHIFT 0x4  /* NOT reference behaviour: w = exp(-(c - min c)/lambda) (underflow-safe) */
#define CCV_MPPI_FLAG_NO_STATE_STORE 0x8 /* skip the K x H x,y state buffer (read_candidates then fails) */

typedef struct ccv_mppi_config {
    int32_t abi_version;        /* CCV_MPPI_ABI_VERSION */
    int32_t model;              /* CCV_MPPI_DIFF_DRIVE ... */
    int32_t num_samples;        /* K on THIS device (param "num_samples", dd:19) */
    int32_t horizon;            /* H: number of states, H-1 control steps (param "horizon", dd:18); 3..CCV_MPPI_MAX_HORIZON */
    int32_t sample_offset;      /* global id of local sample 0 when K is sharded over devices (0 otherwise);
                                 * 0 <= sample_offset and sample_offset + num_samples <= 2^31 - 1, else CCV_MPPI_ERR_INVALID_ARG */
    int32_t device;             /* HIP device ordinal */
    int32_t flags;              /* CCV_MPPI_FLAG_* */
    int32_t reserved;
    double control_noise;       /* sigma, one value for every control dimension (dd:20) */
    double lambda;              /* dd:21 */
    double v_ref;               /* dd:28 */
    double u_min[CCV_MPPI_MAX_UDIM]; /* clamp bounds per control dimension (dd:22-26, sd:23-28, fb:13-26) */
    double u_max[CCV_MPPI_MAX_UDIM];
    double path_weight;         /* dd:33 */
    double v_weight;            /* dd:34 ("control_weight" in dd/sd, "v_weight" in fb:35) */
    double zmp_weight;          /* fb:36 */
    double roll_v_weight;       /* fb:37 */
    double back_weight;         /* fb:38 */
    double yaw_weight;          /* fb:39 */
} ccv_mppi_config;

typedef struct ccv_mppi_stats {
    double sum_w;        /* sum_i exp(-cost_i/lambda) (unnormalised; 0 => u* is NaN exactly like dd:222) */
    double min_cost;
    double max_cost;
    int64_t n_zero_weight; /* samples whose weight underflowed to exactly 0 */
    int32_t nonfinite;   /* 1 if any component of the returned controls is NaN/Inf */
    int32_t reserved;
    float device_us;     /* device time of the last iteration's kernels (hipEvent), 0 if not measured */
    float rollout_us;    /* device time of the dominant kernel (sample+rollout+cost) */
} ccv_mppi_stats;

typedef struct ccv_mppi_handle ccv_mppi_handle;

/* ---- lifetime ------------------------------------------------------------------------------------ */
/* Replaces the allocation part of the constructors (dd:36-46, sd:38-48, fb:72-84). */
int ccv_mppi_create(const ccv_mppi_config* cfg, ccv_mppi_handle** out);
int ccv_mppi_destroy(ccv_mppi_handle* h);
/* Launch on a caller-owned HIP stream (hipStream_t passed as void*); NULL restores the handle's own stream. */
int ccv_mppi_set_stream(ccv_mppi_handle* h, void* hip_stream);
const char* ccv_mppi_last_error(const ccv_mppi_handle* h);
const char* ccv_mppi_version(void);
int ccv_mppi_udim(int model);

/* ---- warm start: optimal_solution controls, layout [(H-1)][u_dim] (dd.h:100) -------- */
int ccv_mppi_set_nominal(ccv_mppi_handle* h, const double* u);
int ccv_mppi_get_nominal(ccv_mppi_handle* h, double* u);

/* ---- one whole iteration: sampling + predict_States + calc_Weights + determine_OptimalSolution ---- */
/* x0: (x, y, yaw[, roll, pitch]) = current_pose_/current_state_ (dd:115-117, fb:458-464); dt: dt_ (dd:347);
 * x_ref/y_ref: the H window points written by calc_RefPath() (dd:156-181); yaw_ref0: yaw_ref_[0] (fb:408);
 * seed/iter: counter-based noise key (the reference reseeds mt19937 from random_device every call, dd:83-84);
 * u_opt_out: new optimal_solution controls [(H-1)][u_dim]; stats may be NULL. Blocking. */
int ccv_mppi_iterate(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref, const double* y_ref,
                     double yaw_ref0, uint64_t seed, uint64_t iter, double* u_opt_out, ccv_mppi_stats* stats);
/* Same work, enqueued on the stream without any host synchronisation; u* stays resident on the device as the
 * next call's warm start.  Read it back with ccv_mppi_get_nominal(). */
int ccv_mppi_iterate_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref,
                             const double* y_ref, double yaw_ref0, uint64_t seed, uint64_t iter);
int ccv_mppi_synchronize(ccv_mppi_handle* h);

/* ---- stage-wise mirrors of the four reference methods (reference call order; parity tests) -------- */
int ccv_mppi_sample(ccv_mppi_handle* h, uint64_t seed, uint64_t iter);                 /* sampling() */
/* Parity hook: overwrite the sample controls with caller data [K][(H-1)][u_dim] (already clamped, e.g. the
 * output of the reference's own sampling()); replaces ccv_mppi_sample for that iteration. */
int ccv_mppi_inject_controls(ccv_mppi_handle* h, const double* u_samples);
int ccv_mppi_rollout(ccv_mppi_handle* h, const double* x0, double dt);                  /* predict_States() */
int ccv_mppi_weights(ccv_mppi_handle* h, const double* x_ref, const double* y_ref, double yaw_ref0); /* calc_Weights() */
int ccv_mppi_update(ccv_mppi_handle* h, double* u_opt_out, ccv_mppi_stats* stats);     /* determine_OptimalSolution() */

/* ---- read-back ------------------------------------------------------------------------------------ */
/* Feeds publish_CandidatePath() (dd:265-294) without a K x H device-to-host copy: samples first, first+stride, ...
 * (count of them); xy_out layout [count][H][2]. */
int ccv_mppi_read_candidates(ccv_mppi_handle* h, int32_t first, int32_t count, int32_t stride, double* xy_out);
/* The `count` samples with the largest weights of the last cost evaluation, in descending order of weight (ties: lower
 * sample index first; NaN weights first, by sample index among themselves): their indices, optionally their unnormalised weights [count] and their rollouts
 * [count][H][2].  Selection (radix select) and gather run on the device; only the selected rows cross PCIe.  This is
 * what publish_CandidatePath() (dd:265-294) can sensibly show of K = 65 536 candidates. */
int ccv_mppi_read_top_candidates(ccv_mppi_handle* h, int32_t count, int32_t* sample_out, double* weight_out, double* xy_out);
int ccv_mppi_read_costs(ccv_mppi_handle* h, int32_t first, int32_t count, double* out);
/* normalised weights w_i / sum_w, i.e. the reference's weights_ (dd:222) */
int ccv_mppi_read_weights(ccv_mppi_handle* h, int32_t first, int32_t count, double* out);
/* sample controls, layout [count][(H-1)][u_dim] */
int ccv_mppi_read_controls(ccv_mppi_handle* h, int32_t first, int32_t count, double* out);

/* ---- K sharded over several devices (one handle per device/process) ------------------ */
/* Number of doubles in the per-device partial vector: 1 + (H-1)*u_dim = [sum w, sum w*u[t][d] ...]. */
int ccv_mppi_partials_size(const ccv_mppi_handle* h);
/* sample+rollout+cost+local reduction; leaves the unnormalised partials in dev_partials (DEVICE memory of this
 * handle's device, e.g. a torch tensor) without touching u*.  The caller all-reduces (sum) dev_partials across
 * devices (RCCL) on the same stream, then calls ccv_mppi_apply_partials on every device. No host sync. */
int ccv_mppi_iterate_partials_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref,
                                      const double* y_ref, double yaw_ref0, uint64_t seed, uint64_t iter,
                                      double* dev_partials);
/* u* = partials[1:] / partials[0] becomes the resident warm start (no host sync).  The division is deferred into the
 * next ccv_mppi_iterate*_enqueue on this handle (one kernel launch less per iteration); dev_partials must stay valid and
 * unchanged until then, or until ccv_mppi_synchronize / ccv_mppi_get_nominal, which perform it at once. */
int ccv_mppi_apply_partials_enqueue(ccv_mppi_handle* h, const double* dev_partials);

/* Same, without a collective-library call per iteration, for the devices of ONE node (world <= 8): each handle owns a
 * small box in its HBM that the peers map (hipIpc over xGMI); the update kernel writes this device's partial vector
 * straight into every peer's box, waits for the peers' vectors in its own and adds them in rank order (identical bits on
 * every device); the division is deferred into the next rollout as above.  Set-up: every process calls _create, the
 * processes exchange the returned handles (ccv_mppi_exchange_handle_bytes() bytes each, e.g. torch.distributed
 * all_gather), then every process calls _connect with all of them in rank order.  Every rank must then issue the same
 * sequence of ccv_mppi_iterate_exchange_enqueue calls; a peer that does not arrive within 10 s yields NaN controls, not a
 * hang, and the next ccv_mppi_synchronize / ccv_mppi_get_nominal on that handle returns CCV_MPPI_ERR_TIMEOUT (the *_enqueue
 * calls themselves cannot know).  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose driver only supports dmabuf IPC.
 * The box is fine-grained (device-coherent) memory; where that cannot be allocated or exported it falls back to ordinary
 * device memory, which _connect accepts only if every rank's box lives on the same physical device (a one-device
 * rehearsal) and refuses with CCV_MPPI_ERR_STATE otherwise -- the caller then takes the all-reduce path above.
 * Handles of one process (one process driving several devices) connect to each other directly, without hipIpc.
 * The blob a rank hands out also carries a nonce; rank 0's is the base of the packet sequence numbers, so a job that is
 * started again does not mistake packets of an earlier one for its own. */
int ccv_mppi_exchange_handle_bytes(void);
int ccv_mppi_exchange_create(ccv_mppi_handle* h, int32_t world, int32_t rank, void* ipc_handle_out);
int ccv_mppi_exchange_connect(ccv_mppi_handle* h, const void* ipc_handles);
/* What was set up (any pointer may be NULL): world, rank, whether this handle's box is fine-grained memory, whether
 * _connect has succeeded. */
int ccv_mppi_exchange_info(const ccv_mppi_handle* h, int32_t* world, int32_t* rank, int32_t* fine_grained, int32_t* connected);
int ccv_mppi_iterate_exchange_enqueue(ccv_mppi_handle* h, const double* x0, double dt, const double* x_ref,
                                      const double* y_ref, double yaw_ref0, uint64_t seed, uint64_t iter);

/* ---- device-resident closed loop -------------------------------------------------- */
/* The per-tick prologue of run() on the device: the whole reference path and the pose live in HBM, and every step does
 *   (advance != 0) pose <- pose advanced for dt by the command u*[0] of the previous step (the Euler model of
 *                  predict_NextState(), dd:104-109 / sd:120-125 / fb:445-452: the closed-loop plant, what the robot does
 *                  between two ticks; ccv_mppi_plant_step() in ccv_mppi_host.h is the same arithmetic on the host)
 *   get_CurrentIndex() (dd:126-140) + calc_RefPath() (dd:156-181) from that pose, then the iteration itself
 * with no host data in between: a closed loop costs two kernel launches per tick (the update of a tick is launched together
 * with the prologue of the next one) and no PCIe traffic.  Window, index
 * and pose are bit-identical to ccv_mppi_calc_ref_path() / ccv_mppi_plant_step() on the host; yaw_ref[0] (read by fb:408
 * only) comes from the device atan2 and may differ from libm's in the last place.  v_ref and the horizon are the
 * handle's; `resolution` is the spacing of the path poses (resolution_, dd:160).  Needs the default (cooperative)
 * kernels.
 * dt must be finite and not negative (it is the stride of the window index, dd:160-163; the reference's behaviour for anything
 * else is undefined): CCV_MPPI_ERR_INVALID_ARG otherwise, as from ccv_mppi_calc_ref_path().
 * The plant takes yaw / roll / pitch modulo 2 pi once they leave +-1e4 rad (the real node reads them from tf in [-pi, pi]),
 * identically in ccv_mppi_plant_step(), so a loop of any length stays inside the range of the kernels' branch-free
 * sin/cos.  A step is refused with CCV_MPPI_ERR_STATE -- before the pose is moved -- when the pose angles (as set by
 * _set_pose) or the commands (clamp bounds, and whatever ccv_mppi_set_nominal put into u*) can leave that range (1e5 rad)
 * within one horizon. */
int ccv_mppi_resident_set_path(ccv_mppi_handle* h, const double* path_x, const double* path_y, int32_t n_path,
                               double resolution);
/* state: (x, y, yaw[, roll, pitch]); also restarts the step counter and the trace */
int ccv_mppi_resident_set_pose(ccv_mppi_handle* h, const double* state);
int ccv_mppi_resident_step_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance);
/* K sharded over devices: as ccv_mppi_iterate_partials_enqueue; every device advances the same pose with the same u* */
int ccv_mppi_resident_step_partials_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance,
                                            double* dev_partials);
/* ... or as ccv_mppi_iterate_exchange_enqueue (direct exchange between the devices of one node) */
int ccv_mppi_resident_step_exchange_enqueue(ccv_mppi_handle* h, double dt, uint64_t seed, uint64_t iter, int32_t advance);
/* Synchronises; any output pointer may be NULL.  x_ref / y_ref: H values, the window of the last step. */
int ccv_mppi_resident_read(ccv_mppi_handle* h, double* state, int32_t* current_index, double* x_ref, double* y_ref,
                           double* yaw_ref0, int64_t* steps);
/* The poses of the last steps, oldest first: rows of (x, y, yaw, roll, pitch, current_index); at most max_rows and at
 * most the 8192 most recent.  This is what record_state.py:118-139 logs from tf. */
int ccv_mppi_resident_read_trace(ccv_mppi_handle* h, int32_t max_rows, double* rows, int32_t* n_rows);

/* ---- measurement ----------------------------------------------------------------------------------- */
/* on = 1: every iteration records hipEvents around the dominant kernel and the whole launch sequence; on = n > 1: every
 * n-th iteration only (keeps the event overhead out of a throughput measurement); 0: off.
 * ccv_mppi_timing_read returns the accumulated device times of the recorded iterations since the last reset (it synchronises). */
int ccv_mppi_timing_enable(ccv_mppi_handle* h, int32_t on);
int ccv_mppi_timing_read(ccv_mppi_handle* h, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters,
                         int32_t reset);

/* ---- batch handles: B independent problems in one launch -------------------------------------------------------- */
/* B controllers that share one configuration (model, K = num_samples per instance, H, sigma, lambda, bounds, weights, flags)
 * -- or, after ccv_mppi_batch_set_params, only its model, K, H and flags, each instance with its own sigma, lambda, v_ref,
 * bounds and weights -- and differ in pose, dt, reference window, warm start and noise seed: one call runs all of them with one rollout launch and
 * one update launch -- what a process that serves N robots, or sweeps N scenarios, would otherwise spend N handles and N
 * blocking round trips on.  Instance b computes what a single handle with the same configuration computes for the same
 * (x0[b], dt[b], x_ref[b], y_ref[b], yaw_ref0[b], seed[b], iter) from the same warm start: its noise is that of noise_spec.h
 * with key seed[b] and the local sample index 0 .. K-1; no input of one instance changes any output bit of another.
 * The bits equal the single handle's where both run the same kernel family, which the single handle's selection rule, applied
 * to the batch's B * ceil(K / 64) workgroups of 64 samples, decides (four-wave kernel up to five workgroups per CU, full body
 * one; the one-wave kernel beyond, also where a single full-body handle would run the two-wave kernel).  One instance whose
 * headings can leave the range of the kernels' fast sin / cos sends the whole batch through the plain kernel, one diff-drive
 * instance with |w|max dt > pi/4 through the wide-turn instantiation: the results then agree with the single handle's to
 * rounding.  CCV_MPPI_KERNEL=v1 selects the plain kernel; the environment's other kernel overrides do not apply to batches.
 * Conventions as above: int status, one batch handle per caller thread, the caller's current device is restored. */
#define CCV_MPPI_BATCH_MAX_SAMPLES (1 << 29) /* B * ceil(K / 64) * 64: the kernels index the sample axis with 32-bit byte offsets */
/* ccv_mppi_batch_last_kernel(): the rollout kernel of the last call (FOUR_WAVE / ONE_WAVE / PLAIN, | WIDE: wide-turn form) */
#define CCV_MPPI_BATCH_KERNEL_PLAIN 0
#define CCV_MPPI_BATCH_KERNEL_ONE_WAVE 1
#define CCV_MPPI_BATCH_KERNEL_FOUR_WAVE 4
#define CCV_MPPI_BATCH_KERNEL_WIDE 16
#define CCV_MPPI_BATCH_KERNEL_VARIED 32 /* ORed in: the kernels with per-instance parameters ran (ccv_mppi_batch_set_params) */
#define CCV_MPPI_BATCH_KERNEL_SHIFT 64   /* ORed into ccv_mppi_batch_last_kernel(): the shifted-weight kernels ran */
#define CCV_MPPI_BATCH_KERNEL_OBST 128   /* ORed in: the kernels with the disc-obstacle term ran (ccv_mppi_batch_set_obstacles) */
#define CCV_MPPI_BATCH_KERNEL_MOVING 256 /* ORed in (with OBST): the kernels with moving discs ran (ccv_mppi_batch_set_obstacle_velocities) */
#define CCV_MPPI_BATCH_KERNEL_GRID 512   /* ORed in (with MOVING | OBST): the kernels with the occupancy-grid term ran (ccv_mppi_batch_set_grids) */
#define CCV_MPPI_MAX_OBSTACLES 32        /* discs per instance */
#define CCV_MPPI_GRID_MAX_DIM 32768      /* cells per axis of an occupancy grid */
#define CCV_MPPI_GRID_MAX_CELLS (1 << 26) /* cells per occupancy grid */
#define CCV_MPPI_INFLATE_MAX_RADIUS 64    /* cells: the largest inflation radius of ccv_mppi_batch_set_occupancy */
#define CCV_MPPI_OCC_PATCH_MAX_CELLS (1 << 20) /* cells of one patch of ccv_mppi_batch_update_occupancy_enqueue */
#define CCV_MPPI_OCC_PATCH_SLOTS 4        /* patches whose staging can be in flight before _update_occupancy_enqueue waits */
#define CCV_MPPI_SCAN_MAX_REACH 4096      /* cells: the largest max(|ex - sx|, |ey - sy|) of a ray of ccv_mppi_batch_scan_occupancy_enqueue */

typedef struct ccv_mppi_batch ccv_mppi_batch;

/* batch >= 1; cfg->sample_offset must be 0; CCV_MPPI_FLAG_MIN_SHIFT is refused (CCV_MPPI_ERR_INVALID_ARG: a batch's
 * underflow-safe weights are a mode of the handle, ccv_mppi_batch_set_min_shift, not a creation flag); batch * ceil(K / 64) * 64 <= CCV_MPPI_BATCH_MAX_SAMPLES.  Arguments are checked before
 * any device is touched; without a device: CCV_MPPI_ERR_NO_DEVICE. */
int ccv_mppi_batch_create(const ccv_mppi_config* cfg, int32_t batch, ccv_mppi_batch** out);
int ccv_mppi_batch_destroy(ccv_mppi_batch* b);
int ccv_mppi_batch_set_stream(ccv_mppi_batch* b, void* hip_stream);
int ccv_mppi_batch_synchronize(ccv_mppi_batch* b);
const char* ccv_mppi_batch_last_error(const ccv_mppi_batch* b);
int ccv_mppi_batch_size(const ccv_mppi_batch* b);
int ccv_mppi_batch_last_kernel(const ccv_mppi_batch* b);
/* warm starts, layout [B][(H-1)][u_dim] */
int ccv_mppi_batch_set_nominal(ccv_mppi_batch* b, const double* u);
int ccv_mppi_batch_get_nominal(ccv_mppi_batch* b, double* u);
/* Per-instance parameters: cfgs[B], instance b's configuration.  Its abi_version, model, num_samples, horizon,
 * sample_offset, device and flags must equal the creation configuration's (otherwise CCV_MPPI_ERR_INVALID_ARG, the first
 * offending instance and field in _last_error, the handle unchanged); control_noise, lambda, v_ref, u_min, u_max and the six
 * weights are the instance's own from the next iteration on.  Instance b then computes what a single handle created with
 * cfgs[b] computes for the same inputs and warm start (bit for bit where both run the same kernel family), and no parameter
 * of one instance changes an output bit of another.  The decisions one instance makes for the batch (plain kernel, wide-turn
 * form, the resident loop's stride and angle checks) take each instance's own bounds and v_ref; the two-instruction clamp is
 * chosen per instance.  cfgs == NULL returns to the creation configuration and the shared kernels.  Flushes a pending resident
 * update and may synchronise; warm starts, paths, poses, step counters and traces stay. */
int ccv_mppi_batch_set_params(ccv_mppi_batch* b, const ccv_mppi_config* cfgs);
/* out[B]: every instance's effective configuration (B copies of the creation configuration before any _set_params) */
int ccv_mppi_batch_get_params(ccv_mppi_batch* b, ccv_mppi_config* out);
/* Underflow-safe weights (NOT reference behaviour), a mode of the handle switched at run time: on != 0 -> from the next
 * iteration on every instance weighs its samples with w = exp(-(c - min c) / lambda_b), min c the instance's own smallest cost
 * and lambda_b its own lambda, so an instance with one finite cost always yields a finite u* (an instance whose costs are all
 * infinite, or that has a NaN cost, yields NaN and nonfinite = 1 as without the mode, and only in that instance).  The fused
 * iteration keeps its two launches and writes no controls: every workgroup of 64 samples forms its weights relative to its own
 * minimum cost and the update rescales the workgroup's sums by exp(-(workgroup minimum - instance minimum) / lambda_b); the
 * plain kernel (CCV_MPPI_KERNEL=v1, unbounded headings) is followed by the exact shift, as CCV_MPPI_FLAG_MIN_SHIFT of a single
 * handle.  The mode always runs the per-instance-parameter kernels (_last_kernel: SHIFT | VARIED | family); a handle without
 * _set_params has B copies of its configuration in the table, and _set_params(NULL) in this mode keeps the mode and returns to
 * those.  Results agree with the mode off to rounding wherever the plain weights do not underflow, not bit for bit; on = 0
 * returns to the kernels and the bits of a handle that never switched.  In this mode the statistics mean: min_cost / max_cost
 * as always; sum_w = sum_i exp(-(cost_i - min_cost) / lambda_b), hence >= 1 for a finite min_cost; n_zero_weight = the number
 * of samples whose weight relative to their workgroup's minimum cost is 0, counted in the workgroups whose scale
 * exp(-(workgroup minimum - min_cost) / lambda_b) is not 0, plus every sample of the workgroups whose scale is 0 (plain
 * kernel: the samples whose shifted weight is 0) -- a sample whose two factors are both above 0 while their product would
 * underflow is not counted.  ccv_mppi_batch_read_weights returns the normalised weights as always.  Flushes a pending
 * resident update, like _set_params, and may synchronise; warm starts, paths, poses, step counters, traces and per-instance
 * parameters stay.  _get_min_shift: 0 / 1, or CCV_MPPI_ERR_INVALID_ARG for a null handle. */
int ccv_mppi_batch_set_min_shift(ccv_mppi_batch* b, int32_t on);
int ccv_mppi_batch_get_min_shift(const ccv_mppi_batch* b);
/* Per-instance disc obstacles (NOT reference behaviour; off by default; batch handles only).  Instance b has n[b] discs
 * (ox, oy, r) in world coordinates, static until the next call, and a weight weight[b] >= 0.  For every state p the path term
 * is taken over (the same states, the same step ranges) the cost gains
 *     weight[b] * max( max_j ( r_j^2 - |p - o_j|^2 ), 0 )
 * -- the deepest penetration, not a sum over the discs; a NaN position contributes 0; the caller inflates r by the robot's own
 * radius and a margin.  The term touches the cost only: noise, controls and states keep their bits, an instance with n[b] = 0
 * or weight[b] = 0 keeps every bit of its result, and no disc of one instance changes a bit of another.  A weight large enough
 * to matter pushes costs past 745 lambda, where the plain weights are all 0 and u* is NaN: use ccv_mppi_batch_set_min_shift.
 * xyr: [B][max_n][3], n: [B] counts (0 <= n[b] <= max_n <= CCV_MPPI_MAX_OBSTACLES), weight: [B].  The term always runs the
 * per-instance-parameter kernels (_last_kernel: OBST | VARIED | family, | SHIFT, | WIDE); a handle without _set_params has B
 * copies of its configuration in the table, and _set_params keeps the obstacles.  xyr == NULL or max_n == 0 turns the term off
 * and returns to the kernels, and the bits, that ran before.  A negative or non-finite weight or r, a non-finite centre, n[b]
 * outside [0, max_n] or max_n above the limit: CCV_MPPI_ERR_INVALID_ARG, nothing changes.  Flushes a pending resident update
 * and synchronises, like _set_params; the resident loop sees the discs from the next step on.
 * _get_obstacles: xyr [B][max_n][3] (rows past n[b] zero), n [B], weight [B]; max_n must hold the largest count (all zero / 0
 * while the term is off); any of the three may be NULL. */
int ccv_mppi_batch_set_obstacles(ccv_mppi_batch* b, const double* xyr, const int32_t* n, int32_t max_n, const double* weight);
int ccv_mppi_batch_get_obstacles(ccv_mppi_batch* b, double* xyr, int32_t* n, int32_t max_n, double* weight);
/* Moving discs (NOT reference behaviour; off by default; batch handles only).  Disc j of instance b gets a velocity
 * (vx, vy) in world coordinates, constant over the horizon: state k of a sample -- k dynamics steps after the pose, state 0 the
 * pose itself, row k of ccv_mppi_batch_read_candidates -- is charged against the disc centred at o_j + v_j * (k * dt[b]), dt[b]
 * the dt of the instance's rollout:
 *     weight[b] * max( max_j ( r_j^2 - |p_k - o_j - v_j k dt|^2 ), 0 )
 * over the same states as the static term, the deepest penetration, a NaN position 0.  vxy: [B][max_n][2] for the discs of
 * _set_obstacles, rows at or past an instance's count ignored (max_n below a count: the remaining discs stand still).  A
 * non-NULL table turns the MOVING kernels on (_last_kernel: MOVING | OBST | VARIED | family, | SHIFT, | WIDE), even one of all
 * zeros -- whose results equal the static term's bit for bit; NULL returns to the static kernels and their bits.  A non-finite
 * value or max_n outside [0, CCV_MPPI_MAX_OBSTACLES]: CCV_MPPI_ERR_INVALID_ARG; no discs set: CCV_MPPI_ERR_STATE; nothing
 * changes either way.  _set_obstacles with a new list clears the velocities (a new list has none until it is given some),
 * _set_obstacles(NULL) removes them with the discs, _set_params keeps them.  Discs the fleet term appends stand still.  Flushes a
 * pending resident update and synchronises, like _set_obstacles.
 * _get_obstacle_velocities: vxy [B][max_n][2], the host copy (rows past the count, and everything while none are set: zero). */
int ccv_mppi_batch_set_obstacle_velocities(ccv_mppi_batch* b, const double* vxy, int32_t max_n);
int ccv_mppi_batch_get_obstacle_velocities(ccv_mppi_batch* b, double* vxy, int32_t max_n);
/* Fleet prediction (NOT reference behaviour; off by default): with the fleet term on (ccv_mppi_batch_resident_set_fleet,
 * ccv_mppi_fleet.h), on != 0 makes every neighbour's disc move over the horizon with the velocity that robot had over the last
 * resident tick, v = (position after the tick's advance - position before it) * (1 / dt), formed on the device by the robot's
 * own prologue block (one fp64 subtraction and one multiplication per component; zero when the tick did not advance, when
 * dt = 0, or when a component is not finite) and carried with its position through the double-buffered snapshot; the selection
 * of the neighbours does not change.  While it is on the MOVING kernels run (_last_kernel: MOVING | OBST | ...); the static discs
 * keep the velocities of _set_obstacle_velocities (zero without).  _resident_set_poses and _resident_set_fleet reset every
 * robot's velocity to zero.  The setter gives CCV_MPPI_ERR_STATE while the fleet term is off; turning the fleet term off turns
 * prediction off; prediction off returns to the kernels, and the bits, of a fleet run that never had it.  Flushes a pending
 * resident update and synchronises.  _get_fleet_prediction: 0 / 1, or CCV_MPPI_ERR_INVALID_ARG for a null handle.
 * _read_fleet_velocities: vxy [B][CCV_MPPI_MAX_OBSTACLES][2], the velocity rows the last tick's rollout was charged with, beside
 * the disc rows of _resident_read_fleet (rows past an instance's total count zero; all zero while the static kernels run); a
 * flush point; CCV_MPPI_ERR_STATE while the fleet term is off. */
int ccv_mppi_batch_set_fleet_prediction(ccv_mppi_batch* b, int32_t on);
int ccv_mppi_batch_get_fleet_prediction(const ccv_mppi_batch* b);
int ccv_mppi_batch_read_fleet_velocities(ccv_mppi_batch* b, double* vxy);
/* Occupancy grids (NOT reference behaviour; off by default; batch handles only).  The handle holds n_maps >= 1 maps.  Map m is
 * nx x ny cells of float, row-major with x fastest (cell (ix, iy) at cells[iy * nx + ix]), its corner (origin_x, origin_y) in
 * world coordinates, resolution > 0 the side of a cell, and `outside` the value of everything that is not in a cell.  Instance b
 * uses map map_of[b] (-1: none) with weight[b] >= 0.  For every state the path term is taken over (the same states and step
 * ranges as the disc term: all H for diff drive and steering, the first H - 2 for full body), in state order k = 0, 1, ..., with
 * (x, y) the state AS STORED, the doubles ccv_mppi_batch_read_candidates returns:
 *     inv = 1.0 / resolution                                  (rounded once, on the host)
 *     fx  = (x - origin_x) * inv,  fy = (y - origin_y) * inv    (one subtraction, one multiplication, no FMA)
 *     in  = fx >= 0 && fx < nx && fy >= 0 && fy < ny           (fp64 compares: false for NaN)
 *     v_k = in ? cells[(int)fy * nx + (int)fx] : outside
 *     G   = ((double)v_0 + (double)v_1) + ...                  (fp64, in state order, from 0.0)
 *     cost = fma(weight[b], G, cost_rest)
 * with cost_rest the sample's complete cost without the term: the grid term is added last, as one FMA, before the weight is
 * formed.  A NaN state reads `outside`: that is the one rule for states that are not numbers.  The term touches the cost only:
 * noise, controls and states keep their bits, an instance with map_of[b] = -1 or weight[b] = 0 keeps every bit of its result
 * (G finite), and no map, map_of or weight of one instance changes a bit of another.  Nearest cell only: no interpolation, no
 * integer cells, no rotated maps, no partial updates of a caller's float map -- a new map is a new _set_grids (a map kept as
 * occupancy can be patched in stream order: ccv_mppi_batch_set_occupancy, _update_occupancy_enqueue below).
 * The term always runs the moving-disc kernels' GRID forms (_last_kernel: GRID | MOVING | OBST | VARIED | family, | SHIFT,
 * | WIDE): a handle without discs runs them over an empty disc list, a handle with static discs over a zero velocity table, whose
 * disc term equals the static one bit for bit.  nx, ny in [1, CCV_MPPI_GRID_MAX_DIM], nx * ny <= CCV_MPPI_GRID_MAX_CELLS.
 * _set_grids: maps [n_maps], map_of [B], weight [B]; the cells are copied.  NULL cells, a size out of range, a non-finite or
 * non-positive resolution, a non-finite origin, outside, weight or cell, a negative weight, map_of[b] outside [-1, n_maps):
 * CCV_MPPI_ERR_INVALID_ARG, nothing changes.  maps == NULL or n_maps == 0 turns the term off and returns to the kernels, and the
 * bits, that ran before.  Flushes a pending resident update and synchronises, like _set_obstacles; the resident loop sees the
 * maps from the next step on; _set_params, _set_obstacles, _set_obstacle_velocities, _set_min_shift and the fleet setters keep
 * them.
 * _get_grids: maps [max_maps] (cells returned NULL), *n_maps, map_of [B] (-1 while off), weight [B] (0 while off); any may be
 * NULL; max_maps below the number of maps with maps != NULL: CCV_MPPI_ERR_INVALID_ARG.
 * _read_grid_cells: cells_out [ny * nx] of map `map`, read back from the device. */
typedef struct ccv_mppi_grid { double origin_x, origin_y, resolution; float outside; int32_t nx, ny; const float* cells; } ccv_mppi_grid;
int ccv_mppi_batch_set_grids(ccv_mppi_batch* b, const ccv_mppi_grid* maps, int32_t n_maps, const int32_t* map_of, const double* weight);
int ccv_mppi_batch_get_grids(ccv_mppi_batch* b, ccv_mppi_grid* maps, int32_t max_maps, int32_t* n_maps, int32_t* map_of, double* weight);
int ccv_mppi_batch_read_grid_cells(ccv_mppi_batch* b, int32_t map, float* cells_out);
/* Costmaps inflated on the device (NOT reference behaviour; off by default; batch handles only).  A second source for the
 * maps of the grid term above: instead of float cells the caller gives occupancy, and the device derives the float cells.  Map m
 * has the geometry of ccv_mppi_grid (origin, resolution, nx, ny, outside), uint8 cells (row-major, x fastest), a threshold in
 * [0, 255] and an inflation (radius R in cells, 0 <= R <= CCV_MPPI_INFLATE_MAX_RADIUS; profile [R * R + 1]; free_value):
 *     occ(ix, iy)  = cells[iy * nx + ix] >= threshold               (a cell outside the map is not occupied)
 *     D2(ix, iy)   = min over occupied (jx, jy) of (jx - ix)^2 + (jy - iy)^2      (int32; +inf if there is none)
 *     cost(ix, iy) = D2 <= R * R ? profile[D2] : free_value
 * -- an exact truncated Euclidean distance transform and a table the caller fills (a linear ramp, an exponential decay, a
 * step): the device evaluates no function of the distance, so cost is defined in every bit.  cost is the float cell the GRID
 * kernels read; everything the grid term's comment says holds with these cells, _get_grids and _read_grid_cells included.
 * _set_occupancy: maps [n_maps], inflation [n_maps], map_of [B], weight [B]; cells and profiles are copied.  What _set_grids
 * refuses, a threshold outside [0, 255], a radius outside [0, CCV_MPPI_INFLATE_MAX_RADIUS], a NULL profile, a non-finite profile
 * entry or free_value: CCV_MPPI_ERR_INVALID_ARG, nothing changes.  maps == NULL or n_maps == 0 turns the term off, as
 * _set_grids(NULL) does.  Flushes a pending resident update and synchronises, like _set_grids.  The two sources replace each
 * other: a later _set_grids (maps or NULL) drops the occupancy layers.  _set_params, _set_obstacles, _set_obstacle_velocities,
 * _set_min_shift and the fleet setters keep them.
 * _update_occupancy_enqueue: the w x h rectangle at cell (x0, y0) of map `map` becomes `patch` (row-major, tightly packed,
 * w * h <= CCV_MPPI_OCC_PATCH_MAX_CELLS), and the float cells the change can reach -- the rectangle grown by R, clipped to the
 * map -- are derived again.  Stream-ordered: no synchronisation, no allocation, no flush of a pending resident update; the patch
 * is copied out of the caller's buffer before the call returns; with CCV_MPPI_OCC_PATCH_SLOTS patches in flight the call waits
 * for the oldest one's writer and nothing else.  A rollout enqueued before the call reads the old cells, every rollout enqueued
 * after it the new ones; the call may come between _resident_step_enqueue calls and between _iterate_enqueue calls.  A
 * rectangle not inside the map, w or h < 1, a patch of more cells than the limit (split it, or call _set_occupancy), a NULL
 * patch, map out of range: CCV_MPPI_ERR_INVALID_ARG; no occupancy set: CCV_MPPI_ERR_STATE; nothing changes either way.
 * _get_occupancy: maps [max_maps] (cells NULL) and inflation [max_maps] (profile NULL), *n_maps (0 unless occupancy is set); any
 * may be NULL; max_maps below the number of maps with maps or inflation != NULL: CCV_MPPI_ERR_INVALID_ARG.
 * _read_occupancy: out [ny * nx], the layer of map `map` read back from the device; synchronises (so does _read_grid_cells while
 * occupancy is set); CCV_MPPI_ERR_STATE while no occupancy is set.
 * _roll_occupancy_enqueue: rolling maps.  The windows of n maps (map [n], each map at most once, 1 <= n <= the number of maps)
 * move by whole cells, map[i] by (dx[i], dy[i]).  With `old` and `new` the layer before and after the call:
 *     new(ix, iy) = old(ix + dx, iy + dy)        where (ix + dx, iy + dy) lies inside the map
 *                 = the caller's cell, or fill   elsewhere (the exposed cells)
 *     cx += dx, cy += dy                         (cells moved since _set_occupancy, int64)
 *     origin_x = origin0_x + (double)cx * resolution,  origin_y = origin0_y + (double)cy * resolution
 * with origin0 the origin _set_occupancy was given: the origin is formed from the accumulated cell count by one multiplication
 * and one addition (no FMA), never by repeated addition, so it does not drift.  nx, ny, resolution, outside, threshold and
 * inflation stay.  |dx| >= nx or |dy| >= ny is legal: every cell is exposed then.  After the call the float cells, the layer and
 * the origin of the map are, in every bit, what a fresh _set_occupancy of `new` at the new origin would produce.
 * exposed == NULL: every exposed cell becomes fill, which must be in [0, 255] (with exposed != NULL fill is not read).  Otherwise
 * exposed holds, entry after entry and tightly packed, for each entry first the row strip and then the column strip:
 *     row strip     the min(|dy|, ny) exposed rows over the full width nx, in ascending new-frame iy
 *     column strip  of every remaining row, in ascending iy, its min(|dx|, nx) exposed cells in ascending ix
 * (an entry with dx = dy = 0 has neither).  A 5 x 4 map (nx = 5, ny = 4) rolled by (dx, dy) = (2, -1): row iy = 0 is exposed
 * (dy < 0: the low rows), and in the rows iy = 1, 2, 3 the columns ix = 3, 4 (dx > 0: the high columns), so the entry is
 *     new(0,0) new(1,0) new(2,0) new(3,0) new(4,0)   new(3,1) new(4,1)   new(3,2) new(4,2)   new(3,3) new(4,3)
 * -- 1 * 5 + 3 * 2 = 11 bytes; rolled by (-2, 1) it is row iy = 3 and then the columns ix = 0, 1 of the rows iy = 0, 1, 2.
 * Stream-ordered like _update_occupancy_enqueue: no synchronisation, no flush of a pending resident update; exposed, map, dx
 * and dy may be reused when the call returns.  A rollout enqueued before the call reads the old map at the old origin, every
 * rollout enqueued after it the new one; the call may come between _resident_step_enqueue calls, between _iterate_enqueue calls
 * and between patches, and is two kernel launches however many maps it rolls (none when every shift is zero).  A later
 * _update_occupancy_enqueue addresses the rolled frame; _read_occupancy, _read_grid_cells, _get_grids and _get_occupancy show the
 * rolled map and its origin (the origin from the moment the call returns).  The call stages its tables and strips in one slot of
 * the patches' ring: with m the number of entries that move, 336 * m bytes plus the strips must not exceed
 * CCV_MPPI_OCC_PATCH_MAX_CELLS bytes -- split a larger call by maps, or use _set_occupancy (64 maps of 200 x 200 rolled by
 * (1, 1): 64 * (336 + 399) bytes).  The handle's first roll after a _set_occupancy allocates a second set of layers and float
 * cells of the same size and, that once, flushes and synchronises like a setter: a roll with every dx = dy = 0 is the priming
 * call, which changes no bit; no later roll allocates.  The second set is freed with the layers (_set_occupancy, _set_grids,
 * destroy), and a new _set_occupancy starts again from its own origin with no cell moved.  No occupancy set: CCV_MPPI_ERR_STATE.
 * n out of range, a map out of range or named twice, |dx| or |dy| above CCV_MPPI_GRID_MAX_DIM, an accumulated offset beyond
 * +-2^30 cells, a rolled origin that is not finite, fill out of range, tables and strips above a slot, NULL map, dx or dy:
 * CCV_MPPI_ERR_INVALID_ARG.  Nothing changes either way.
 * _scan_occupancy_enqueue: range scans traced into the layers.  Entry i of the n entries (1 <= n <= the number of maps) names a
 * map map[i] (each map at most once), the sensor's cell (sensor_xy[i][0], sensor_xy[i][1]), which must lie inside the map, and
 * n_rays[i] >= 0 rays; the rays of all entries follow each other, entry after entry, in end_xy [sum n_rays][2] (a ray's end
 * cell, which may lie outside the map) and hit [sum n_rays] (non-zero: the ray ended on something).  All coordinates are int32
 * cells of the map's current frame, the rolled one that _update_occupancy_enqueue addresses.  Integers only.  With (sx, sy) the
 * sensor's cell and (ex, ey) a ray's end cell:
 *     adx = |ex - sx|, ady = |ey - sy|;  the major axis is x if adx >= ady, else y;  a = major length, b = minor length
 *     cell i, 0 <= i < a:  major = s_major + sign_major * i,  minor = s_minor + sign_minor * ((2 * i * b + a) div (2 * a))
 * -- the integer error walk (e = a; per step e += 2b; if e >= 2a: e -= 2a, minor += 1) written per step.  Cell 0 is the
 * sensor's cell; the end cell (i = a) is not part of the ray; a ray with a = 0 has no cells.  The reach a of a ray is at most
 * CCV_MPPI_SCAN_MAX_REACH.  With `old` and `new` the layer before and after the call:
 *     new = old
 *     every ray cell inside the map                                  = clear_value
 *     the end cell, where it lies inside the map, of a ray with hit  = mark_value     (after ALL clears of that map)
 * so marks win over clears within a call, whatever the order of the rays and of the entries; cells outside the map are
 * skipped, never wrapped; clear_value and mark_value, each in [0, 255], are the bytes stored (occupancy is still
 * cells >= threshold).  After the call the layer and the float cells of the map are, in every bit, what a fresh _set_occupancy
 * of `new` would produce: per entry the float cells of one rectangle are derived again -- the bounding box of the sensor cell
 * and all end cells, clipped to the map, grown by R and clipped again.  Stream-ordered like _update_occupancy_enqueue and
 * _roll_occupancy_enqueue: no synchronisation, no allocation, no flush of a pending resident update; every array may be reused
 * when the call returns.  A rollout enqueued before the call reads the old cells, every rollout enqueued after it the new ones;
 * the call may come between _resident_step_enqueue calls, between _iterate_enqueue calls, between patches and rolls, and is two
 * kernel launches however many maps it scans.  An entry with n_rays = 0 takes no room and does no work; a call in which nothing
 * is traced launches nothing.  The call stages its tables and rays in one slot of the patches' ring: 9 bytes per ray (the end
 * cell and the hit byte) and 128 bytes per entry that has rays must not exceed CCV_MPPI_OCC_PATCH_MAX_CELLS bytes -- the largest
 * call of one entry has 116 494 rays, 64 entries of 360 rays take 215 552 bytes; split a larger call by maps, or by rays into
 * calls that all clear and a last one that also marks.  No occupancy set: CCV_MPPI_ERR_STATE.  n out of range, a map out of range
 * or named twice, a sensor cell outside its map, a negative n_rays, a reach above the limit, clear_value or mark_value outside
 * [0, 255], a call that does not fit one slot, NULL map, sensor_xy or n_rays, NULL end_xy or hit with a ray to read:
 * CCV_MPPI_ERR_INVALID_ARG.  Nothing changes either way. */
typedef struct ccv_mppi_occupancy { double origin_x, origin_y, resolution; float outside; int32_t nx, ny, threshold; const uint8_t* cells; } ccv_mppi_occupancy;
typedef struct ccv_mppi_inflation { int32_t radius; float free_value; const float* profile; } ccv_mppi_inflation;
int ccv_mppi_batch_set_occupancy(ccv_mppi_batch* b, const ccv_mppi_occupancy* maps, const ccv_mppi_inflation* inflation, int32_t n_maps,
                                 const int32_t* map_of, const double* weight);
int ccv_mppi_batch_update_occupancy_enqueue(ccv_mppi_batch* b, int32_t map, int32_t x0, int32_t y0, int32_t w, int32_t h, const uint8_t* patch);
int ccv_mppi_batch_roll_occupancy_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* map, const int32_t* dx, const int32_t* dy,
                                          const uint8_t* exposed, int32_t fill);
int ccv_mppi_batch_scan_occupancy_enqueue(ccv_mppi_batch* b, int32_t n, const int32_t* map, const int32_t* sensor_xy /*[n][2]*/,
                                          const int32_t* n_rays /*[n]*/, const int32_t* end_xy /*[sum n_rays][2]*/, const uint8_t* hit /*[sum n_rays]*/,
                                          int32_t clear_value, int32_t mark_value);
int ccv_mppi_batch_get_occupancy(ccv_mppi_batch* b, ccv_mppi_occupancy* maps, ccv_mppi_inflation* inflation, int32_t max_maps, int32_t* n_maps);
int ccv_mppi_batch_read_occupancy(ccv_mppi_batch* b, int32_t map, uint8_t* out);
/* Range sensors simulated on the device (NOT reference behaviour; off until called; batch handles and resident steps only).  The
 * handle holds one ground-truth world map with the geometry of ccv_mppi_occupancy (origin, resolution, nx, ny, threshold, uint8
 * cells; `outside` is not read): a world cell is occupied when cells >= threshold, a cell outside the world is not occupied.  The
 * world is read by the sensor only and is never a cost term.  Every costmap that is sensed into must have the world's resolution
 * bit for bit; per map the caller states an anchor (ax, ay), the world cell that coincided with the map's cell (0, 0) when
 * _set_occupancy was called.  With (cx, cy) the cells the map has rolled since then, the map's cell (0, 0) is the world cell
 * (ax + cx, ay + cy) at call time and local cell = world cell - that offset: no floating point enters the frame change, and the
 * caller answers for the anchor being true (the grid term goes on using the map's own origin).
 * _resident_sense_enqueue: the n named instances (instance [n], each at most once, no two on one map, 1 <= n <= B) sense.  The
 * pose of instance b is its resident pose as the stream finds it -- the pose _resident_read would return at that point, which is
 * the pose the last enqueued tick rolled out from.  Its world cell is the grid term's formula against the world:
 *     inv = 1.0 / resolution                                  (rounded once, on the host)
 *     fx  = (x - origin_x) * inv,  fy = (y - origin_y) * inv    (one subtraction, one multiplication, no FMA)
 *     in  = fx >= 0 && fx < nx && fy >= 0 && fy < ny           (fp64 compares: false for NaN)
 *     s   = ((int)fx, (int)fy)
 * A robot that is not `in` (outside the world, or a NaN pose) senses nothing: no cell of its map changes and its rectangle is
 * empty.  beam_xy [n_beams][2] holds the end offsets (dx, dy) of the beams in cells, |dx|, |dy| <= CCV_MPPI_SCAN_MAX_REACH,
 * world-aligned and shared by all entries (1 <= n_beams <= max_beams).  Beam r of a robot at world cell s runs along
 * _scan_occupancy_enqueue's line from s to e = s + (dx, dy); its cells are i = 0 .. a by the same closed form, cell a being the
 * end cell.  Integers only:
 *     f = min { i in [1, a] : cell i lies inside the world and is occupied }          (the sensor's own cell is not tested)
 *     f exists:  the local cells of i in [0, f) = clear_value,  local cell f = mark_value     (after ALL clears of that map)
 *     otherwise: the local cells of i in [0, a) = clear_value,  nothing is marked
 * The cleared cells are a prefix of the beam's own line, not the line re-traced to cell f.  Local cells outside the map are
 * skipped, never wrapped; the sensor's local cell may lie outside its map.  clear_value and mark_value are per call, each in
 * [0, 255].  After the call the layer and the float cells of every sensed map are, in every bit, what a fresh _set_occupancy of
 * the new layer would produce: per entry one rectangle is derived again -- the box s_local + [min dx, max dx] x [min dy, max dy]
 * clipped to the map, grown by R and clipped again, min and max taken over the beam table and the offset (0, 0), so that the
 * box holds the sensor cell and every end cell.  Stream-ordered like the three _occupancy_enqueue calls: no synchronisation,
 * no allocation, no flush of a pending resident update; every array may be reused when the call returns; two kernel launches
 * however many robots sense.  Beams and entry table share one slot of the patches' ring: 8 bytes per beam and 112 bytes per
 * entry must not exceed CCV_MPPI_OCC_PATCH_MAX_CELLS bytes.  No world set, or no resident poses set: CCV_MPPI_ERR_STATE.  n or
 * n_beams out of range, an instance out of range or named twice, an instance without a map, two named instances on one map
 * (split the call: a later call's marks win over an earlier call's clears), a map whose resolution differs from the world's, an
 * offset ax + cx or ay + cy beyond +-2^30, a reach above the limit, a value outside [0, 255], a call that does not fit a slot,
 * NULL arrays: CCV_MPPI_ERR_INVALID_ARG.  Nothing changes either way.
 * _resident_read_sense: the simulated scan itself.  first [B][max_beams] int32: f of beam r of instance b's last sensing, or -1
 * where the beam was not blocked or the robot sensed nothing (-1 everywhere before an instance's first sensing and past the
 * beams of its last call); sensor_cell [B][2]: the robot's world cell, or (-1, -1) where it sensed nothing.  Only the rows of
 * instances named by a call are written.  Synchronises, as _read_occupancy does; either pointer may be NULL.
 * _set_world: world (cells copied) and anchor_xy [n_maps][2] for the maps of _set_occupancy, max_beams in
 * [1, CCV_MPPI_SENSE_MAX_BEAMS]; a setter like _set_occupancy: flushes a pending resident update and synchronises.  No occupancy
 * set: CCV_MPPI_ERR_STATE.  A size out of range, a non-finite origin or resolution, a threshold outside [0, 255], max_beams out
 * of range, NULL cells or anchors, an anchor beyond +-2^29: CCV_MPPI_ERR_INVALID_ARG.  world == NULL drops the world; so do a
 * later _set_occupancy and _set_grids (the anchors speak of those layers) and destroy; the other setters keep it.
 * _get_world: the geometry (cells NULL), anchor_xy [max_maps][2] and *max_beams; any may be NULL; CCV_MPPI_ERR_STATE while no
 * world is set; max_maps below the number of maps with anchor_xy != NULL: CCV_MPPI_ERR_INVALID_ARG.
 * _read_world: out [ny * nx], the world read back from the device; synchronises.
 * _update_world_enqueue: the w x h rectangle at cell (x0, y0) of the world becomes `patch`, in stream order and in one launch,
 * with the refusals of _update_occupancy_enqueue: the ground truth can change under a running fleet (a door closes). */
#define CCV_MPPI_SENSE_MAX_BEAMS 4096     /* beams of one ccv_mppi_batch_resident_sense_enqueue */
int ccv_mppi_batch_set_world(ccv_mppi_batch* b, const ccv_mppi_occupancy* world, const int32_t* anchor_xy /*[n_maps][2]*/, int32_t max_beams);
int ccv_mppi_batch_get_world(ccv_mppi_batch* b, ccv_mppi_occupancy* world /*cells NULL*/, int32_t* anchor_xy, int32_t max_maps, int32_t* max_beams);
int ccv_mppi_batch_read_world(ccv_mppi_batch* b, uint8_t* out);
int ccv_mppi_batch_update_world_enqueue(ccv_mppi_batch* b, int32_t x0, int32_t y0, int32_t w, int32_t h, const uint8_t* patch);
/* (ccv_mppi_batch_resident_sense_enqueue and ccv_mppi_batch_resident_read_sense are declared in ccv_mppi_sense.h, included below.) */
/* x0 [B][5] (x, y, yaw[, roll, pitch]; unused entries ignored), dt [B], x_ref / y_ref [B][H], yaw_ref0 [B], seed [B];
 * u_opt_out [B][(H-1)][u_dim]; stats [B] or NULL.  Blocking: the result arrives through the pinned mailbox, B * (R + 4) slots. */
int ccv_mppi_batch_iterate(ccv_mppi_batch* b, const double* x0, const double* dt, const double* x_ref, const double* y_ref,
                           const double* yaw_ref0, const uint64_t* seed, uint64_t iter, double* u_opt_out, ccv_mppi_stats* stats);
/* the same work without a host synchronisation; u* stays resident as the next call's warm start (ccv_mppi_batch_get_nominal) */
int ccv_mppi_batch_iterate_enqueue(ccv_mppi_batch* b, const double* x0, const double* dt, const double* x_ref, const double* y_ref,
                                   const double* yaw_ref0, const uint64_t* seed, uint64_t iter);
/* per-instance read-backs of the last iteration, as ccv_mppi_read_costs / _read_weights / _read_candidates */
int ccv_mppi_batch_read_costs(ccv_mppi_batch* b, int32_t instance, int32_t first, int32_t count, double* out);
int ccv_mppi_batch_read_weights(ccv_mppi_batch* b, int32_t instance, int32_t first, int32_t count, double* out);
int ccv_mppi_batch_read_candidates(ccv_mppi_batch* b, int32_t instance, int32_t first, int32_t count, int32_t stride,
                                   double* xy_out);
/* What a node publishes per robot (publish_CandidatePath(), publish_OptimalPath(); dd:265-312), for every instance at once.
 * Selection, ordering, gather and the re-roll run on the device; each call takes one synchronisation and one device-to-host copy
 * per output array, sorts nothing on the host and copies nothing to the device.
 * _read_best_candidates: the `count` lowest-cost samples of EVERY instance of the last tick.  sample_out [B][count] (local sample
 * index 0..K-1), cost_out [B][count] (may be NULL), xy_out [B][count][H][2] (may be NULL; layout per candidate as
 * ccv_mppi_batch_read_candidates).  Selection is by cost, not by weight: the same order as descending weight wherever the weights
 * are distinct and positive, and defined where they are not -- where weights underflow to 0, and under
 * ccv_mppi_batch_set_min_shift, where the stored weights are relative to their workgroup.  Costs ascend, ties go to the lower
 * sample index, NaN costs come last, by index among themselves: the order of one 64-bit key (every NaN 0xFFFFFFFFFFFFFFFF, -0.0
 * as +0.0, otherwise bits ^ (sign ? ~0 : 1 << 63)) and then the index, i.e. of numpy's lexsort((arange(K), cost)).  cost_out
 * holds the costs' own bits.  Only samples 0..K-1 take part.  The call reads costs and states only: it does not flush a pending
 * resident update and runs in stream order after the rollout launch, so a resident tick keeps its two launches.  Works with every
 * form of a batch and every kernel family.  count == 0 is OK and writes nothing.  A null handle or sample_out, count < 0,
 * count > K or count > CCV_MPPI_BEST_MAX: CCV_MPPI_ERR_INVALID_ARG; before any tick, or xy_out with
 * CCV_MPPI_FLAG_NO_STATE_STORE: CCV_MPPI_ERR_STATE (indices and costs still work with that flag).
 * _read_optimal_paths: the plant model rolled through every instance's u* from the pose and dt of the last tick: xyyaw_out
 * [B][H-1][3], row i = the state BEFORE control step i (dd:295-312, as MPPIBase::optimal_path()), bit for bit H-1 calls of
 * ccv_mppi_plant_step().  Needs u*, so it flushes a pending resident update as ccv_mppi_batch_get_nominal does.  A null handle
 * or xyyaw_out: CCV_MPPI_ERR_INVALID_ARG; before any tick: CCV_MPPI_ERR_STATE. */
#define CCV_MPPI_BEST_MAX 1024   /* candidates per instance of one call */
int ccv_mppi_batch_read_best_candidates(ccv_mppi_batch* b, int32_t count, int32_t* sample_out, double* cost_out, double* xy_out);
int ccv_mppi_batch_read_optimal_paths(ccv_mppi_batch* b, double* xyyaw_out);
/* as ccv_mppi_timing_enable / _read: the rollout kernel of the whole batch and the whole launch sequence */
int ccv_mppi_batch_timing_enable(ccv_mppi_batch* b, int32_t on);
int ccv_mppi_batch_timing_read(ccv_mppi_batch* b, double* rollout_us_sum, double* iter_us_sum, int64_t* n_iters, int32_t reset);

/* ---- batch handles: device-resident closed loop of every instance ---------------------------------------------------- */
/* The device-resident closed loop above for all B instances of a batch handle at once: every instance has a path, a pose, a
 * noise key, a step counter and a trace of its own in HBM, and one step runs every instance's prologue (plant, index,
 * window) and writes the instance's record -- what ccv_mppi_batch_iterate copies from the host -- on the device.  A tick
 * costs two launches however large B is (the update of a tick is launched together with the prologue of the next one) and
 * no host data.  Instance b's index, window, pose and u* are bit-identical to ccv_mppi_calc_ref_path() +
 * ccv_mppi_plant_step() on the host driving ccv_mppi_batch_iterate; yaw_ref[0] comes from the device atan2 (as above).
 * Kernel selection is the batch's (ccv_mppi_batch_create), without the plain kernel: a step that would need it
 * (CCV_MPPI_KERNEL=v1, pose angles or commands of some instance that can leave the fast sin / cos's range) is refused with
 * CCV_MPPI_ERR_STATE, a bad dt, or a window stride v_ref * dt / resolution[b] that is not usable, with
 * CCV_MPPI_ERR_INVALID_ARG -- in both cases before any pose moves.  Every other call on the batch handle (warm starts,
 * ccv_mppi_batch_iterate*, the read-backs, synchronisation, streams, new paths or poses, destroy) first launches a pending
 * update, so resident steps and host-record iterations may be mixed: each sees the other's u*.  The noise key of instance b
 * is seed[b] of _set_poses; a step passes the iteration number only, and dt is one for all instances. */
#define CCV_MPPI_BATCH_TRACE_ROWS 1024 /* rows of every instance's trace ring: 48 KB per instance */
/* B paths back to back: instance b's n_path[b] >= 1 poses start at sum(n_path[0..b)); resolution [B] > 0 */
int ccv_mppi_batch_resident_set_paths(ccv_mppi_batch* b, const double* path_x, const double* path_y, const int32_t* n_path,
                                      const double* resolution);
/* state [B][5] (x, y, yaw[, roll, pitch]), seed [B] (the noise key of every later step; the step passes iter);
 * restarts every instance's step counter and trace.  After _set_paths. */
int ccv_mppi_batch_resident_set_poses(ccv_mppi_batch* b, const double* state, const uint64_t* seed);
/* one tick of every instance, one dt for all; no host data, no synchronisation */
int ccv_mppi_batch_resident_step_enqueue(ccv_mppi_batch* b, double dt, uint64_t iter, int32_t advance);
/* synchronises; any pointer may be NULL: state [B][5], index [B], x_ref / y_ref [B][H] (the last step's windows),
 * yaw_ref0 [B], steps (shared: the steps since _set_poses) */
int ccv_mppi_batch_resident_read(ccv_mppi_batch* b, double* state, int32_t* current_index, double* x_ref, double* y_ref,
                                 double* yaw_ref0, int64_t* steps);
/* one instance's last rows, oldest first, (x, y, yaw, roll, pitch, index); at most max_rows and at most
 * CCV_MPPI_BATCH_TRACE_ROWS */
int ccv_mppi_batch_resident_read_trace(ccv_mppi_batch* b, int32_t instance, int32_t max_rows, double* rows, int32_t* n_rows);
/* The fleet term of the resident loop -- the robots of one batch keep clear of each other,
 * ccv_mppi_batch_resident_set_fleet / _get_fleet / _read_fleet -- is declared in ccv_mppi_fleet.h, included below. */
/* Paths planned on the device (NOT reference behaviour; off until called; batch handles and resident steps only): the six calls
 * ccv_mppi_batch_resident_set_plan / _get_plan / _plan_enqueue / _read_plan / _read_plan_field / _read_path are declared in
 * ccv_mppi_plan.h, included below.  What they promise.  Instance b plans on its own map (of _set_grids or _set_occupancy, in the
 * current, rolled frame; nx x ny float cells) from the cell its resident pose lies in to a goal cell.  Integers only, but for one
 * pose-to-cell step and one cell-to-pose step:
 *     blocked(c) = !(cell(c) <= lethal)    an fp32 compare: a NaN cell is blocked, a cell equal to lethal is free; everything
 *                                          outside the map is blocked
 *     moves      (x, y) -> (x + dx, y + dy), dx, dy in {-1, 0, 1}, not both zero; a straight move has weight 5, a diagonal move
 *                weight 7; a move is allowed iff the target is not blocked, and a diagonal move also needs (x + dx, y) and
 *                (x, y + dy) both not blocked (no corner cutting; the rule is symmetric)
 *     field      D uint16: 65535 on blocked cells, D(goal) = 0, elsewhere min(65533, least total weight of an allowed path to
 *                the goal); 65533 means both "not reached" and "farther than 65532".  D is the one fixpoint of
 *                D(c) = min(D(c), min(65533, D(n) + w)), whatever order the device relaxes in
 *     start      fx = (x - origin_x) * inv, fy likewise (the grid term's formula against the map's own origin as rolled: one
 *                subtraction, one multiplication, no FMA); in = fx >= 0 && fx < nx && fy >= 0 && fy < ny; s = ((int)fx, (int)fy);
 *                the pose is the resident pose as the stream finds it, as for the sensor: the host reads no pose
 *     descent    from c = s until D(c) == 0: the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with
 *                D(n) + w == D(c).  L = the cells visited, start and goal included
 *     pose i     the centre of cell i: x = origin_x + ((double)ix + 0.5) * resolution (one multiplication, one addition, no FMA),
 *                y likewise; pose 0 is the start cell.  Diagonal poses are sqrt(2) * resolution apart, straight ones
 *                resolution: the window stride of the prologue counts poses, so a planned window is up to sqrt(2) longer.
 * Status per instance, the first that applies: CCV_MPPI_PLAN_NO_START (not `in`, or a NaN pose), _START_BLOCKED, _GOAL_BLOCKED,
 * _NOT_CONVERGED (no sweep without a change within max_sweeps), _UNREACHABLE (D(s) == 65533), _TRUNCATED (L > capacity[b]), _OK;
 * 0: the instance has never planned.  On _OK and _TRUNCATED the first min(L, capacity[b]) poses replace the instance's path and
 * n_path becomes that count; on every other status no bit of the path, n_path or the next tick changes.  A sweep relaxes every
 * free cell at least once against values at least as new as the end of the previous sweep; the call converges whenever
 * max_sweeps >= J, the sweeps of a Jacobi iteration including its last one that changes nothing (nx * ny + 1 is always enough);
 * below J the outcome is the device's own.  (nx + 2)(ny + 2) <= CCV_MPPI_PLAN_MAX_FIELD: the field lives in one CU's LDS.  The
 * instance's path resolution must equal its map's resolution bit for bit, so the stride check of _resident_step_enqueue stays
 * true whether or not a plan succeeds.
 * _set_plan: capacity [B], each in [0, CCV_MPPI_PLAN_MAX_POSES] (0: the instance does not plan); a setter: flushes a pending
 * resident update and synchronises.  Comes after _resident_set_paths (CCV_MPPI_ERR_STATE before).  The paths are laid out again
 * with room for max(n_path[b], capacity[b]) poses per instance and the present paths copied: no bit of any tick changes.  With
 * keep_fields one field of CCV_MPPI_PLAN_MAX_FIELD uint16 is kept per instance that has capacity.  capacity == NULL turns
 * planning off (the paths stay as they are); so does a later _resident_set_paths; destroy frees everything.  While planning is
 * set, _resident_set_poses keeps every instance's path, planned or not.
 * _plan_enqueue: the n named instances (instance [n], each at most once, 1 <= n <= B; two may share a map, which is only read)
 * plan to goal_xy [n][2], in stream order and in one kernel launch: no synchronisation, no allocation, no flush of a pending
 * resident update, no copy; every array may be reused when the call returns.  It may come between steps, patches, rolls, scans
 * and sensings; the next tick's prologue finds the new path.  Planning not set, or no resident poses: CCV_MPPI_ERR_STATE.  n out
 * of range, an instance out of range or named twice, an instance without a map or with capacity 0, a goal outside the map, a
 * map above the size limit, a resolution mismatch, a NaN lethal, max_sweeps outside [1, CCV_MPPI_PLAN_MAX_FIELD], NULL arrays:
 * CCV_MPPI_ERR_INVALID_ARG.  Nothing changes either way.
 * _read_plan: per instance the status, poses (L, or 0 without a descent), start_cell [B][2] ((-1, -1) for _NO_START and before
 * the first plan), start_dist (D(s), or -1 where the field did not converge or was not built) and the sweeps taken, of its last
 * plan; synchronises; any pointer may be NULL.  _read_plan_field: out [ny][nx], instance's field of its last plan; synchronises;
 * CCV_MPPI_ERR_STATE without keep_fields or while the instance's last status is not 1, 2 or 6.  _read_path: the instance's current
 * path, planned or set: *n_path and the first min(n_path, max_poses) poses; synchronises. */
/* Paths planned on the device: traversal weights (NOT reference behaviour; off until called; batch handles and resident steps
 * only): the two calls ccv_mppi_batch_resident_set_plan_penalty / _get_plan_penalty are declared in ccv_mppi_plan_cost.h,
 * included below.  What they promise.  Everything above stands -- blocked, the eight moves, no corner cutting, the uint16 field
 * with 65535 and 65533, the start cell, the status order, the pose formula -- and two handle-wide values, gain and max_penalty,
 * give every free cell a multiplier from its own float value:
 *     t = cell(c) * gain                    one fp32 multiplication, round to nearest, no FMA
 *     q(c) = !(t > 0) ? 0 : (t >= (float)max_penalty ? max_penalty : (int)t)      truncation; a NaN t gives 0
 *     m(c) = 1 + q(c)                       1..16
 *     step(c -> n) = w(c, n) * m(c)         w = 5 straight, 7 diagonal: the cell that is left is charged, not the cell entered
 *     field      the one fixpoint of D(c) = min(D(c), min(65533, D(n) + step(c -> n))) over allowed moves, D(goal) = 0: the
 *                least total charge of a path from c to the goal, every cell on it but the goal charged, the start included;
 *                the move rule is no longer symmetric: D is the charge to the goal, not from it
 *     descent    the first allowed neighbour in the order E, N, W, S, NE, NW, SW, SE with D(n) + step(c -> n) == D(c)
 * Any relaxation order reaches the same integers, and the call converges whenever max_sweeps >= J, the sweeps of the weighted
 * Jacobi iteration; D still falls by at least 5 a step, so CCV_MPPI_PLAN_MAX_POSES holds every path.  With max_penalty == 0 or
 * gain == 0 every multiplier is 1: the plan is the unweighted one in every bit, from the same kernel as before.
 * _set_plan_penalty: gain finite and >= 0, max_penalty in [0, CCV_MPPI_PLAN_MAX_PENALTY]; a NaN, infinite or negative gain or a
 * max_penalty outside the range: CCV_MPPI_ERR_INVALID_ARG, and nothing changes.  Needs _resident_set_plan
 * (CCV_MPPI_ERR_STATE otherwise).  Host state only: no synchronisation, no allocation, no launch; it holds for every later
 * _plan_enqueue and _plan_goals_enqueue, which stay one kernel launch (two while the maps follow).  A fresh _set_plan starts at
 * (0, 0); the setting is dropped with planning: _set_plan(NULL), _resident_set_paths, destroy.  _read_plan, _read_plan_field,
 * _read_path, keep_fields and the status values are what they were and report the weighted plan.
 * _get_plan_penalty: the values as the library holds them; either pointer may be NULL. */
/* Costmaps that follow their robots (NOT reference behaviour; off until called; batch handles and resident steps only): the five
 * calls ccv_mppi_batch_resident_set_follow / _get_follow / _follow_enqueue / _read_follow / _plan_goals_enqueue are declared in
 * ccv_mppi_follow.h, included below.  What they promise.  The window of a device-inflated costmap (_set_occupancy) is re-centred
 * on the resident pose of its robot in stream order, decided on the device: the host reads no pose.  For a named instance b with
 * map m = map_of[b], the map's frame as the stream finds it (cx, cy, origin_x, origin_y) and the resident pose (x, y):
 *     fx = (x - origin_x) * inv,  fy likewise     (the grid term's formula: inv = RN(1 / resolution), the host's; one subtraction,
 *                                                  one multiplication, no FMA)
 *     ok = fabs(fx) < 2^30 && fabs(fy) < 2^30     (false for a NaN or infinite pose)
 *     px = (int64)floor(fx), py likewise          (floor, not truncation: the pose may lie left of or below the map)
 *     ex = px - nx / 2,  ey = py - ny / 2         (C integer division: the centre cell)
 *     dx = |ex| <= margin ? 0 : clamp(ex, -max_step, max_step),  dy likewise, each axis on its own
 *     cx' = cx + dx, cy' = cy + dy;  |cx'| > 2^30 or |cy'| > 2^30, or a rolled origin not finite: nothing moves
 *     origin' = origin0 + (double)cx' * resolution    (one multiplication, one addition, no FMA: the host roll's formula)
 *     status: CCV_MPPI_FOLLOW_MOVED, _HELD (dx = dy = 0), _NO_POSE (not ok), _LIMIT; 0: the map has never been followed
 * On _MOVED the map is rolled by (dx, dy) with every exposed cell set to `fill`: the layer, the float cells, the instances' grid
 * rows and the origin equal in every bit what ccv_mppi_batch_roll_occupancy_enqueue(m, dx, dy, exposed = NULL, fill) leaves, by
 * that call's own promise a fresh _set_occupancy of the rolled layer.  On every other status no bit of the layer, the float cells,
 * the origin or any tick changes.  Whatever the status, a named map changes to its second set of buffers (a copy where nothing
 * moves): the host cannot know which maps moved.
 * While following is set, the device's frame is the truth.  _resident_sense_enqueue keeps its meaning (the anchor plus the cells
 * the map has rolled) and _resident_plan_enqueue its own (goal cells in the rolled frame, the same refusals; start cell and poses
 * from the origin as rolled), each with one small launch more that completes its table on the device; _update_occupancy_enqueue
 * and _scan_occupancy_enqueue address the rolled frame as the device has it; _roll_occupancy_enqueue returns CCV_MPPI_ERR_STATE
 * (the windows are the device's to move); _get_grids, _get_occupancy and _read_follow synchronise and show the device's frame;
 * _set_occupancy, _set_grids and destroy drop following.  A sensing does not check the frame offset against 2^30 on the host: the
 * device holds |cx| <= 2^30 and the anchor is at most 2^29.
 * _set_follow: a setter: flushes a pending resident update and synchronises.  Needs occupancy (CCV_MPPI_ERR_STATE otherwise).
 * on != 0 allocates the second set of layers and cells if no roll has yet, the frame table seeded from the host's (cx, cy,
 * origin) and the result rows; on = 0 reads the frames back into the host's layers and frees the part: host rolls work again
 * and no bit of any tick changes.  _get_follow: *on = whether following is set.
 * _follow_enqueue: the n named instances (instance [n], each at most once, 1 <= n <= B, each on a map of its own) follow, in
 * stream order and in two kernel launches however many: no synchronisation, no allocation, no flush of a pending resident update,
 * no copy; the array may be reused when the call returns.  n outside [1, B], an instance out of range or named twice, an instance
 * without a map, two named instances on one map, margin outside [0, CCV_MPPI_GRID_MAX_DIM], max_step outside
 * [1, CCV_MPPI_GRID_MAX_DIM], fill outside [0, 255], tables above one staging slot, NULL arrays: CCV_MPPI_ERR_INVALID_ARG.
 * Following not set, or no resident poses: CCV_MPPI_ERR_STATE.  Nothing changes either way.
 * _read_follow: per map the status and shift [n_maps][2] = (dx, dy) of its last call ((0, 0) unless _MOVED), and the current
 * frame: offset [n_maps][2] = (cx, cy), origin [n_maps][2]; synchronises; any pointer may be NULL.
 * _plan_goals_enqueue: _plan_enqueue with world goals goal_xy [n][2] as doubles, for a caller who cannot know the frame: the
 * device turns each into a cell against the origin as rolled, f = (p - origin) * inv clamped to the map (f < 0 -> 0,
 * f >= n -> n - 1, else (int)f); a goal that is not finite: CCV_MPPI_ERR_INVALID_ARG.  Everything else is _plan_enqueue's.
 * Following not set: CCV_MPPI_ERR_STATE (a caller who knows the frame has _plan_enqueue). */

#ifdef __cplusplus
}
#endif
#include "ccv_mppi_fleet.h"
#include "ccv_mppi_sense.h"
#include "ccv_mppi_plan.h"
#include "ccv_mppi_follow.h"
#include "ccv_mppi_plan_cost.h"
#endif /* CCV_MPPI_H_ */

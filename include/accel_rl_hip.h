/*
 * accel_rl_hip.h -- C-ABI of libaccel_rl_hip.so (hand-written HIP for gfx950 / MI355X).
 *
 * The reference (astooke/accel_rl) is pure Python and has NO FFI boundary of its
 * own; its hot path is Python/numpy loops and Theano graphs.  The
 * entry points below are what a binding for that path would bind: one function
 * per reference routine on the path, each citing the reference code it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes stub
 * a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (no allocation
 *     inside, no torch types); sizes are plain integers;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only ENQUEUES work on it and is hipGraph-capturable;
 *   - return value: 0 = ok; < 0 = argument error (ARL_E_*); > 0 = hipError_t of
 *     the failed launch.  arl_last_error() returns a thread-local message;
 *   - batch arrays are "env-major": flat index = env * horizon + t
 *     (accel_rl/buffers/batch.py:59-76);
 *   - results: integer / byte / index outputs are bit-exact with the reference;
 *     floating point follows the reference's own dtype walk (see `promo`).
 */
#ifndef ACCEL_RL_HIP_H
#define ACCEL_RL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARL_ABI_VERSION 5

#define ARL_E_ARG      (-1)   /* null pointer / non-positive size                 */
#define ARL_E_RANGE    (-2)   /* size outside what the kernels support             */
#define ARL_E_ALIGN    (-3)   /* pointer not aligned as documented                 */

/* numpy promotion the reference arithmetic is reproduced under:
 * NEP50  = numpy >= 2 (python float x float32 -> float32), bit-exact with the
 *          reference as it runs today;
 * LEGACY = numpy 1.x (python float x float32 scalar -> float64), as in 2018;
 * ASSOC  = (scans only) LEGACY's operand types with the recurrence evaluated as a wavefront suffix scan of affine
 *          maps instead of a sequential walk: f64 sums are reassociated, results agree with both exact modes to
 *          1e-5 (the tolerance BASELINE.json states for returns / advantages) but not bit for bit.  Used for
 *          horizons of 96 .. 512 steps, where it is the faster kernel; others take the LEGACY walk.            */
#define ARL_PROMO_NEP50   0
#define ARL_PROMO_LEGACY  1
#define ARL_PROMO_ASSOC   2

int         arl_abi_version(void);
const char* arl_last_error(void);

/* ------------------------------------------------------------------------- *
 * Return / advantage scans
 * ------------------------------------------------------------------------- */

/* GAE(lambda).  Replaces gen_adv_est, accel_rl/algos/pg/util.py:6-23, and the
 * per-env Python loop around it, accel_rl/algos/pg/aac_base.py:122-127.
 *   rewards, values  f32[n_env*horizon]   dones u8[n_env*horizon] (0/1)
 *   last_values      f32[n_env]           (bootstrap V, aac_base.py:112)
 *   advantages, returns  f32[n_env*horizon] (out; may not alias the inputs)   */
int arl_gae_scan(const float* rewards, const float* values, const uint8_t* dones,
                 const float* last_values, double discount, double gae_lambda,
                 int64_t n_env, int32_t horizon, int32_t promo,
                 float* advantages, float* returns, void* stream);

/* n-step discounted return + advantage.  Replaces discount_returns,
 * accel_rl/algos/pg/util.py:26-37, and `adv[:] = ret - v`, aac_base.py:115-121. */
int arl_nstep_return(const float* rewards, const uint8_t* dones, const float* values,
                     const float* last_values, double discount,
                     int64_t n_env, int32_t horizon, int32_t promo,
                     float* returns, float* advantages, void* stream);

/* valids mask + zeroing.  Replaces update_valids / zero_after_reset,
 * accel_rl/algos/pg/util.py:40-63 (loop at aac_base.py:129-134).
 *   reset_flags u8[n_env*horizon] = env_infos.need_reset if present else dones
 *   valids i8[n_env*horizon] (out); advantages/returns/values are zeroed IN
 *   PLACE after the first set flag (any of the three may be NULL).            */
int arl_valids_mask(const uint8_t* reset_flags, int64_t n_env, int32_t horizon,
                    int8_t* valids, float* advantages, float* returns, float* values,
                    void* stream);

/* (adv - mean) / (std + eps), population std, over all n samples or over the
 * valid ones.  Replaces accel_rl/algos/pg/aac_base.py:136-143.
 *   workspace: >= arl_standardize_workspace_bytes() bytes of device scratch.  */
int64_t arl_standardize_workspace_bytes(void);
int arl_standardize(float* advantages, const int8_t* valids_or_null, int64_t n,
                    double eps, void* workspace, void* stream);

/* ------------------------------------------------------------------------- *
 * Categorical action sampling
 * ------------------------------------------------------------------------- */

/* k = #{j : cumsum_j(prob[b,:]) < u[b]} clamped to n_actions-1; fp32 sequential
 * cumsum, fp64 compare.  Replaces weighted_sample_n, rllab/misc/special.py:22-27
 * (called from accel_rl/spaces/discrete.py:67-68 and
 * accel_rl/policies/pg/atari_cnn_policy.py:110).  The uniform variates the
 * reference draws with np.random.rand(B) are an explicit input.
 *   prob f32[batch*n_actions]  uniforms f64[batch]  actions u8[batch] (out)    */
int arl_sample_categorical(const float* prob, const double* uniforms,
                           int64_t batch, int32_t n_actions, uint8_t* actions,
                           void* stream);

/* ------------------------------------------------------------------------- *
 * Vectorised environment step (synthetic fixed-frame emulator + AtariEnv
 * wrapper + collector bookkeeping)
 * ------------------------------------------------------------------------- */

#define ARL_MAX_ACTIONS 18
#define ARL_TICKET_SHARDS 16
#define ARL_EPOCH_WORDS (32 * (ARL_TICKET_SHARDS + 1))
#define ARL_RAW_H 210
#define ARL_RAW_W 160
#define ARL_OBS_H 104     /* accel_rl/envs/atari_env.py:13 */
#define ARL_OBS_W 80

/* How the cropped 208 x 160 maximum of two raw frames becomes the 104 x 80 observation plane
 * (accel_rl/envs/atari_env.py:155: `cv2.resize(self._max_frame[:-2], (W, H), cv2.INTER_NEAREST)`).  In cv2's Python
 * signature resize(src, dsize[, dst[, fx[, fy[, interpolation]]]]) the constant lands in the `dst` slot, so what
 * RUNS is the default INTER_LINEAR, which for an exact 2x decimation is the rounded 2x2 box (a+b+c+d+2)>>2:
 * ARL_RESAMPLE_BOX2X, the default and the parity mode.  ARL_RESAMPLE_NEAREST is what the call NAMES (and what a
 * reference with the argument fixed would compute): dst(y, x) = src(2y, 2x), OpenCV's floor(dst * scale) rule.
 * OpenCV (opencv3=3.1.0, environment.yml:24) is not under /root/reference: both restated, parity unpinned.        */
#define ARL_RESAMPLE_BOX2X    0
#define ARL_RESAMPLE_NEAREST  1

/* Static description of one game + AtariEnv constructor arguments
 * (accel_rl/envs/atari_env.py:18-26).  Plain data, passed by pointer (host). */
typedef struct arl_game {
    const uint8_t* bank;        /* device u8[n_frames][210][160] frame bank      */
    int32_t n_frames;
    int32_t n_actions;
    int32_t action_set[ARL_MAX_ACTIONS]; /* ALE action codes (getMinimalActionSet)*/
    int32_t start_lives;
    int32_t life_period;
    int32_t frame_skip;         /* atari_env.py:20 */
    int32_t n_stack;            /* num_img_obs, atari_env.py:21 */
    int32_t clip_reward;        /* atari_env.py:22 */
    int32_t episodic_lives;     /* atari_env.py:23 */
    int32_t resample_mode;      /* ARL_RESAMPLE_*; atari_env.py:155 (0 = what the reference computes) */
} arl_game;

/* Per-env mutable state, struct-of-arrays; every pointer is device memory of
 * n_env elements unless noted.  Allocated and owned by the caller. */
typedef struct arl_env_state {
    int64_t  n_env;
    int32_t* tick;          /* emulator frames since reset_game                  */
    int32_t* emu_lives;     /* ale.lives()                                       */
    int32_t* env_lives;     /* AtariEnv._lives (atari_env.py:179)                */
    int32_t* phase;         /* per-emulator frame-bank phase                     */
    uint8_t* over;          /* ale.game_over()                                   */
    uint8_t* frozen;        /* NonResetCollector need_reset[i] (worker.py:75-95) */
    /* TrajInfo accumulators (accel_rl/sampler/util.py:75-101) */
    int32_t* traj_len;
    int32_t* traj_nonzero;
    float*   traj_ret;
    float*   traj_raw;
    float*   traj_disc;
    double*  traj_curdisc;
    /* per-step hand-off from arl_env_act_step to arl_env_frame_step */
    int32_t* frame_a;       /* bank index of raw_frame_1, -1 = all-zero frame    */
    int32_t* frame_b;       /* bank index of raw_frame_2                          */
    uint8_t* frame_mode;    /* 0 skip, 1 shift+push, 2 blank+push                 */
    uint8_t* reset_flag;    /* env must be reset by arl_env_frame_step            */
    /* start-noop streams: one per simulated worker process
     * (accel_rl/envs/atari_env.py:97 draws from the worker's numpy RNG)       */
    const uint8_t* noop_ring;   /* u8[n_streams][noop_ring_len] pre-drawn counts */
    int64_t* noop_cursor;       /* i64[2][n_streams], ping-pong by epoch parity  */
    int32_t* epoch;             /* i32[ARL_EPOCH_WORDS], zero-initialised: [0] number of env launches so far;
                                 * [2] arl_env_step's count of resets its one-launch-ahead forecast (next_reset) did
                                 * not announce -- must stay 0, a caller should check it once per batch;
                                 * the rest are arl_env_step's arrival tickets ([1] top, [32 (s + 1)] shard s: one
                                 * 128-byte line each when the array is 128-byte aligned) */
    int32_t  noop_ring_len;
    int32_t  envs_per_stream;
    /* completed-trajectory records (the reference's traj_infos_queue,
     * overlap/worker.py:147-148): appended with an atomic counter            */
    int32_t* done_count;        /* i32[1]                                        */
    int32_t* done_int;          /* i32[done_capacity][3] = env, Length, NonzeroRewards */
    float*   done_flt;          /* f32[done_capacity][3] = Return, RawReturn, DiscountedReturn */
    int32_t  done_capacity;
    /* arl_env_step only (both may be NULL for the two-launch path).
     * next_reset: u8[2][n_env], ping-pong by the parity of launch_count; [p][e] != 0 <=> env e will be flagged
     * for a mid-batch reset by its next step.  Written by arl_env_step and arl_env_reset for the launch that
     * follows; arl_env_act_step / arl_env_frame_step do not maintain it (after using them, reset every env with
     * arl_env_reset before the next arl_env_step).
     * launch_count: i32[1], arl_env_step / arl_env_reset launches on THIS state (the epoch above may be shared
     * with another state that draws from the same no-op streams, e.g. a worker's evaluation envs).          */
    uint8_t* next_reset;
    int32_t* launch_count;
} arl_env_state;

/* Rollout batch buffer, env-major (accel_rl/sampler/act_server/buffers.py:7-38).
 * Optional arrays may be NULL (raw_reward when !clip_reward, need_reset when
 * !episodic_lives: the reference's env_infos then lack the key).               */
typedef struct arl_rollout {
    int32_t  horizon;
    uint8_t* observations;  /* u8[n_env*horizon][n_stack][104][80]               */
    float*   rewards;       /* f32[n_env*horizon]                                */
    uint8_t* dones;         /* u8 (bool)                                         */
    float*   raw_reward;    /* env_infos.raw_reward                              */
    uint8_t* need_reset;    /* env_infos.need_reset                              */
    uint8_t* actions;       /* u8                                                */
    float*   prob;          /* agent_infos.prob f32[n_env*horizon][n_actions]    */
    float*   value;         /* agent_infos.value                                 */
    uint8_t* step_obs;      /* u8[n_env][n_stack][104][80] current observation   */
} arl_rollout;

/* One agent step for every env, scalar part (one lane per env): sample the
 * action, write actions/prob/value at index env*horizon+step, advance the
 * emulator frame_skip times, apply reward clipping / episodic-life / over-length
 * / reset rules, accumulate TrajInfo, write rewards/dones/env_infos.
 * Replaces: serve_actions' sample+scatter, overlap/sampler.py:139-145;
 * AtariEnv.step minus pixels, envs/atari_env.py:65-78,165-191;
 * ResetCollector / NonResetCollector.collect bookkeeping, overlap/worker.py:37-59,
 * 75-106; TrajInfo.step, sampler/util.py:92-101.
 *   prob f32[n_env][n_actions], value f32[n_env], uniforms f64[n_env] for THIS step
 *   active_or_null u8[n_env]: envs with 0 sit this step out untouched (used for the
 *   start-up decorrelation of sampler/util.py:34-57); NULL = every env steps    */
int arl_env_act_step(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                     const float* prob, const float* value, const double* uniforms,
                     const uint8_t* active_or_null,
                     int32_t step, int32_t mid_batch_reset, double max_path_length,
                     double discount, void* stream);

/* Pixel part (one workgroup per env): resolve pending resets (start no-ops from
 * the env's stream, in env order within the stream), max of the two raw frames,
 * crop 2 rows, rounded 2x2 box to 104x80, shift/blank the frame stack, write
 * step_obs and observations[env*horizon + step + 1] (if step+1 < horizon).
 * Replaces AtariEnv._update_obs/_reset_obs/reset, envs/atari_env.py:93-100,
 * 151-163, and the observation writes of overlap/worker.py:51-53.
 *   max_start_noops: atari_env.py:24                                          */
int arl_env_frame_step(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                       int32_t step, int32_t max_start_noops, void* stream);

/* arl_env_act_step + arl_env_frame_step as ONE launch (one workgroup per env; lane 0 does the scalar rules,
 * the workgroup the pixels, the last workgroup to finish advances the launch epoch): the env side of one agent
 * step of serve_actions / ResetCollector.collect, overlap/sampler.py:129-145, overlap/worker.py:37-59,75-106,
 * envs/atari_env.py:65-78,93-100,151-191.  Same arguments and results as the two calls in sequence.
 * Needs st->next_reset and max_path_length >= 1.
 *   single_write != 0 (needs mid_batch_reset != 0 and active_or_null == NULL): the new stacked observation is
 *   written once -- to observations[env*horizon + step + 1], or to step_obs after the last step of the batch --
 *   and the previous stack is read from observations[env*horizon + step] (which the caller has filled for
 *   step 0, overlap/worker.py:30-32); step_obs is then only current after the last step.  In this mode
 *   observations and step_obs must be 16-byte aligned (ARL_E_ALIGN otherwise; 8-byte alignment suffices without). */
int arl_env_step(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                 const float* prob, const float* value, const double* uniforms,
                 const uint8_t* active_or_null, int32_t step, int32_t mid_batch_reset,
                 double max_path_length, double discount, int32_t max_start_noops,
                 int32_t single_write, void* stream);

/* Start of a batch: observations[env * horizon + 0] = step_obs[env] for every env (the collectors' first row,
 * overlap/worker.py:30-32) and st->done_count[0] = 0 (a fresh traj_infos queue), in one launch.                  */
int arl_rollout_begin(const arl_game* game, const arl_env_state* st, const arl_rollout* ro, void* stream);

/* Reset every env whose flag is set (u8[n_env]; NULL = all): start_envs with
 * max_decorrelation_steps == 0 (sampler/util.py:26-33) and
 * NonResetCollector.reset_needed_envs (overlap/worker.py:108-113, flags =
 * st->frozen, cleared afterwards).  Writes step_obs only.                      */
int arl_env_reset(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                  const uint8_t* flags_or_null, int32_t max_start_noops, void* stream);

/* Stand-alone preprocess of explicit raw frame pairs (testing / other
 * emulators): out[i] = resample(crop(max(a[i], b[i]))), resample_mode = ARL_RESAMPLE_BOX2X (the reference's
 * arithmetic) or ARL_RESAMPLE_NEAREST; a may be NULL (zeros).
 * Replaces envs/atari_env.py:151-155.  a,b u8[n][210][160], out u8[n][104][80] */
int arl_preprocess_frames(const uint8_t* raw_a_or_null, const uint8_t* raw_b,
                          int64_t n, int32_t resample_mode, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Learner side: minibatch gather and the flat-bucket optimiser step
 * ------------------------------------------------------------------------- */

/* dst[0 .. nbytes) = src[0 .. nbytes) as a KERNEL (capturable as a kernel node).  The one exception to "device
 * pointers only": either side may be PINNED host memory (hipHostMalloc / a pinned torch tensor), which the device
 * addresses directly -- this is how the per-batch host hand-offs (action uniforms, minibatch permutations, lr
 * multiplier in; episode records, gradient norms out: the reference's shared-memory step buffers and queues,
 * sampler/act_server/buffers.py:24-30, optimizers/util.py:8-18) enter and leave the hipGraphs without memcpy nodes.
 * A write to host memory is visible to the host once the stream has passed an event / synchronisation after it.   */
int arl_copy_bytes(void* dst, const void* src, int64_t nbytes, void* stream);
/* ring[(counter[0] % n_slots)][0 .. n) = src[0 .. n); counter[0] = (counter[0] + 1) % n_slots (kept reduced) -- the per-iteration diagnostics of an update
 * (the opt_infos of accel_rl/algos/pg/aac_base.py:104-106, e.g. GradNorm) leave a captured hipGraph into a slot the host
 * can name without a launch of its own (it counts the replays).  ring f32[n_slots][n], counter i32[1] on the device. */
int arl_ring_append(const float* src, int32_t n, float* ring, int32_t n_slots, int32_t* counter, void* stream);

/* Rows of up to ARL_GATHER_MAX_ITEMS arrays gathered by ONE shared index vector in ONE launch: for every item,
 * dst row j (j = 0 .. n_rows - 1) = src row map(idx[j]) (idx NULL: map(j)).  This is how the learner's first minibatch
 * takes over the activations the rollout's forwards have just computed under the same parameters, instead of computing
 * them again (the reference re-evaluates the whole network on `s[idxs]`, accel_rl/optimizers/util.py:86-89).
 *   row_map  how the sources are laid out (NULL = ARL_ROW_MAP_IDENTITY).  IDENTITY: map(r) = r.  STEP_MAJOR: the sources
 *            were written step-major [horizon][n_env] while the rows are named env-major, r = env * horizon + t (the
 *            batch arrays' convention above): map(r) = (r % horizon) * n_env + r / horizon.
 *   Loads and stores are 16 bytes wide: row_bytes a positive multiple of 16, <= 2^30 (else ARL_E_RANGE), src and dst 16-byte and idx
 *   4-byte aligned (else ARL_E_ALIGN).  Also refused, nothing launched: items NULL, a NULL src or dst, src_rows < 1
 *   (ARL_E_ARG); n_items outside 1 .. ARL_GATHER_MAX_ITEMS, n_rows outside 1 .. 2^31 - 1, src_rows > 2^31 - 1, a kind other
 *   than the two, STEP_MAJOR with horizon < 1, n_env < 1 or horizon * n_env > 2^31 - 1, and -- the one case in which the
 *   host knows the indices -- idx NULL with a row outside a source: n_rows > src_rows, or STEP_MAJOR with n_rows >
 *   horizon * n_env or horizon * n_env > src_rows (ARL_E_RANGE).  idx itself lives on the device: the kernel cannot
 *   refuse a bad entry, so a mapped source row outside [0, src_rows) reads row 0 (as arl_conv2d_u8_fwd does with
 *   obs_rows), never memory outside the source.  dst must not overlap any src.                                       */
typedef struct arl_gather_item {
    const void* src;        /* [src_rows][row_bytes] */
    void*       dst;        /* [n_rows][row_bytes]   */
    int64_t     row_bytes;
    int64_t     src_rows;
} arl_gather_item;
#define ARL_GATHER_MAX_ITEMS 8
#define ARL_ROW_MAP_IDENTITY   0
#define ARL_ROW_MAP_STEP_MAJOR 1
typedef struct arl_row_map {
    int32_t kind;           /* ARL_ROW_MAP_* */
    int32_t horizon;        /* STEP_MAJOR: T */
    int32_t n_env;          /* STEP_MAJOR: N */
    int32_t reserved;
} arl_row_map;
int arl_gather_rows_many(const arl_gather_item* items, int32_t n_items, const int32_t* idx_or_null, int64_t n_rows,
                         const arl_row_map* row_map_or_null, void* stream);

/* out[b] = float(obs[idx[b]]) * scale  (u8 -> f32 gather; the reference gathers
 * on device with `s[idxs]`, accel_rl/optimizers/util.py:86-89, and scales by
 * 1/255 in ScalarFixedScaleLayer, accel_rl/policies/layers.py:22-41).
 *   obs u8[n_rows][row_bytes], idx i32[batch] (NULL = identity), out f32[batch][row_bytes] */
int arl_gather_scale_obs(const uint8_t* obs, const int32_t* idx_or_null, int64_t batch,
                         int64_t row_bytes, float scale, float* out, void* stream);

/* Channels-last variant of arl_gather_scale_obs for the conv stack:
 * obs u8[n_rows][channels][plane_bytes] -> out f32[batch][plane_bytes][channels].
 * channels must be 4 (the 4-frame stack, atari_env.py:21), plane_bytes % 16 == 0. */
int arl_gather_scale_obs_nhwc(const uint8_t* obs, const int32_t* idx_or_null, int64_t batch,
                              int32_t channels, int32_t plane_bytes, float scale, float* out,
                              void* stream);

/* A minibatch of whole trajectory segments for a recurrent policy, prepared in ONE launch from the segment numbers
 * (the second value of iterate_traj_idxs, accel_rl/optimizers/util.py:21-32).  The batch is [n_traj_total][horizon]
 * rows, segment-major.
 *   idx[j * horizon + t]  = seg[j] * horizon + t                  the chosen segments' rows in time order
 *   state_out[s][j][:]    = state_in[s][seg[j] * horizon][:]      the stored state BEFORE step 0 of each chosen
 *                                                                 segment (aac_base.py:157-161: only s[::horizon])
 *   inv_count[0]          = 1 / #{rows r of idx : valids[r] != 0} as f32; the count is an integer sum, so the result
 *                           has the same bits every run.  No valid row at all gives 0 (never inf / NaN).  Without
 *                           valids every row counts: 1 / (n_seg * horizon).
 *   seg i32[n_seg]; state_in / state_out: HOST arrays of n_state (0 .. 2) device pointers, f32
 *   [n_traj_total * horizon][hidden] and f32 [n_seg][hidden], 16-byte aligned (else ARL_E_ALIGN; both may be NULL
 *   with n_state == 0); valids i8[n_traj_total * horizon] or NULL; idx i32[n_seg * horizon]; inv_count f32[1] or
 *   NULL (not computed).  Segment numbers may repeat.
 * The CALLER guarantees 0 <= seg[j] < n_traj_total: the numbers live on the device, the host cannot check them and
 * the kernel clamps nothing (and asserts nothing).
 * Null pointers: ARL_E_ARG.  ARL_E_RANGE, nothing launched and no output written: n_seg < 1, horizon < 1,
 * n_traj_total < 1, n_state outside 0 .. 2, hidden % 4 != 0, hidden > 1024, n_seg * horizon > 2^31 - 1 or
 * n_traj_total * horizon > 2^31 - 1 (row numbers are int32).  One workgroup per segment: a latency-bound launch.  */
int arl_traj_minibatch(const int32_t* seg, int32_t n_seg, int32_t horizon, int64_t n_traj_total,
                       const float* const* state_in, int32_t n_state, int32_t hidden,
                       const int8_t* valids_or_null, int32_t* idx, float* const* state_out,
                       float* inv_count_or_null, void* stream);

/* x[rows][channels] = relu(x + bias[c]) in place: the bias + rectify of Lasagne's
 * Conv2DLayer / DenseLayer (accel_rl/policies/pg/networks/pg_cnn.py:47-68) on a
 * channels-last activation.  channels % 4 == 0.                                 */
int arl_bias_relu(float* x, const float* bias, int64_t rows, int32_t channels, void* stream);

/* Backward of the above: dy *= (y > 0) in place, dbias[c] = sum_rows dy (fixed
 * summation order).  workspace >= arl_relu_bwd_workspace_bytes().               */
int64_t arl_relu_bwd_workspace_bytes(void);
int arl_relu_bwd_bias_grad(float* dy, const float* y, int64_t rows, int32_t channels,
                           float* dbias, void* workspace, void* stream);
/* Deferred folds.  The weight-gradient and bias-gradient kernels write per-split partial sums; the
 * *_parts entry points stop there and describe the pending fold in *item (splits == 0: `out` is already
 * final), so that a whole backward pass ends in ONE arl_fold_many launch instead of one small fold
 * kernel per tensor.  Each item needs its own workspace region, live until arl_fold_many has run;
 * out[i] = sum_z part[z*total + i] in a fixed order (bit-reproducible). */
typedef struct arl_fold_item {
    const float* part;      /* f32[splits][total] */
    float*       out;       /* f32[total], 16-byte aligned */
    int64_t      total;     /* multiple of 4 */
    int32_t      splits;
    int32_t      valid;     /* > 0: `out` holds only this many floats (the partials are padded to `total`); 0 = total */
} arl_fold_item;
#define ARL_FOLD_MAX_ITEMS 24

/* Same, leaving the column-sum fold to arl_fold_many (see arl_fold_item). */
int arl_relu_bwd_bias_parts(float* dy, const float* y, int64_t rows, int32_t channels, float* dbias,
                            void* workspace, arl_fold_item* item, void* stream);

/* Policy / value heads + softmax for action serving: prob = softmax(h W_pi^T + b),
 * value = h w_v + b_v.  Replaces the output layers of _f_prob_value,
 * accel_rl/policies/pg/atari_cnn_policy.py:63-67 (pg_cnn.py:70-86).
 *   h f32[batch][hid]; w_head f32[n_actions+1][hid] (rows 0..A-1 pi, row A value);
 *   b_head f32[n_actions+1]; prob f32[batch][A]; value f32[batch]
 * Limits (else ARL_E_RANGE, nothing launched): 1 <= n_actions <= ARL_MAX_ACTIONS (18), 1 <= hid <= 1024,
 * 1 <= batch <= 2^31 - 1.  Any hid in range (64, 256, 512 and 1024 have specialised kernels).                  */
int arl_pg_head_infer(const float* h, const float* w_head, const float* b_head, int64_t batch,
                      int32_t hid, int32_t n_actions, float* prob, float* value, void* stream);

/* Training-time heads: forward, the three losses and every gradient up to dh in
 * one pass.  kind 0 = A2C  pi_loss = -mean(log(pi[a]+1e-8) adv)    (a2c.py:43-46)
 *            kind 1 = PPO  pi_loss = -mean(min(r adv, clip(r, 1 -+ clip_param*lr_mult) adv)),
 *                          r = (pi[a]+1e-8)/(old[a]+1e-8)          (ppo.py:42-51)
 * v_loss = c_v mean((V-R)^2); ent_loss = -c_e mean(-sum pi log(pi+1e-8))
 * (aac_base.py:60-66, categorical.py:66-78); means are valids_mean when valids
 * is given (algos/pg/util.py:49-53; inv_count = 1/sum(valids) over the minibatch).
 * Rows of the batch arrays are selected by idx (NULL = identity).
 * tie_rule (PPO only) = how min() and clip() hand their gradient on (s1 = r adv, s2 = clip(r) adv, surr = min(s1, s2)):
 *   ARL_PPO_TIE_THEANO  the reference learner's graph as its Theano differentiates it.  accel_rl runs on
 *                       theano.gpuarray (runners/accel_rl_base.py:62-64; algos/dqn/cat_dqn.py:85-86 names
 *                       "Theano 0.9" / "1.0"), i.e. Theano >= 0.9; since 0.8 theano/scalar/basic.py has
 *                           Minimum.L_op:  e = eq(min, x);  gx = e gz;  gy = (1 - e) gz
 *                           ("This form handle the case when both value are the same. In that case, gx will be
 *                            gz, gy will be 0."; theano/tensor/tests/test_basic.py::test_maximum_minimum_grad:
 *                            "we only pass the gradient to the first input in that case")
 *                           Clip.L_op:     gx = ((x >= min) & (x <= max)) gz
 *                       and ppo.py:49 is T.minimum(surr_1, surr_2), so
 *                           d surr / d r = adv [surr == s1] + adv [surr != s1] [lo <= r <= hi]:
 *                       adv inside the clip range (the tie goes to the unclipped branch alone) and where s1 < s2
 *                       outside it, else 0.  Theano is a third-party dependency absent from /root/reference:
 *                       restated from its published source, parity unpinned.
 *   ARL_PPO_TIE_MATH    the mathematical derivative: adv inside the range, adv where s1 < s2 outside, else 0 (differs
 *                       from the above only where s1 == s2 by rounding OUTSIDE the range).
 *   ARL_PPO_TIE_BOTH    Theano <= 0.7 (gx = eq(min, x) gz, gy = eq(min, y) gz: a tie feeds BOTH arguments):
 *                       2 adv inside the clip range, bounds included; for comparing against runs of that vintage.
 *   out: dout f32[batch][A+1], dh f32[batch][hid] (before the hidden relu mask),
 *        dw_head f32[A+1][hid], db_head f32[A+1], loss4 f32[4] = pi, v, ent, pi+v+ent
 *        (dw_head, db_head, loss4 16-byte aligned: arl_fold_many writes them)
 *   workspace >= arl_pg_head_workspace_bytes()
 * Limits as arl_pg_head_infer (n_actions <= 18, hid <= 1024, 1 <= batch <= 2^31 - 1; else ARL_E_RANGE before any
 * launch).  The head kernel's LDS holds w_head ((A+1) hid floats, up to 76 KiB) and, while (A+1) hid <= 3 072,
 * four slices of the weight gradient; past 64 KiB it opts in to the larger size per launch.  The separate weight
 * gradient kernel (larger (A+1) hid) stages dout in fixed row chunks: its LDS does not grow with the batch.       */
#define ARL_PPO_TIE_THEANO 0
#define ARL_PPO_TIE_MATH   1
#define ARL_PPO_TIE_BOTH   2
int64_t arl_pg_head_workspace_bytes(void);
int arl_pg_head_loss(const float* h, const float* w_head, const float* b_head,
                     const uint8_t* actions, const float* advantages, const float* returns,
                     const float* old_prob, const int8_t* valids_or_null,
                     const int32_t* idx_or_null, const float* lr_mult,
                     const float* inv_count_or_null, int64_t batch, int32_t hid, int32_t n_actions,
                     int32_t kind, int32_t tie_rule, float clip_param, float v_loss_coeff, float ent_loss_coeff,
                     int32_t relu_mask_dh, float* dout, float* dh, float* dw_head, float* db_head,
                     float* loss4, void* workspace, void* stream);
/* Same, stopping before the three small folds (dw_head, db_head, loss4): they are described in items3[0..2] for
 * arl_fold_many, so that a backward pass ends in ONE fold launch.  The bias partials are n_actions + 1 rounded
 * up to a multiple of 4 floats in the partials only (items3[1].valid = n_actions + 1), and so are the weight partials,
 * (n_actions + 1) * hid of them per split (items3[0].valid = (n_actions + 1) * hid where that is not a multiple of 4,
 * else 0); workspace stays live until the fold has run.
 * wt_items_or_null / n_wt (ABI 4): the same launch also writes these layers' k-contiguous weight copies
 * (arl_conv2d_dgrad_weights below) in extra workgroups -- the backward pass that follows reads them, and this launch is
 * where a minibatch's parameters are final and the CUs are idle: one launch less per minibatch.                     */
int arl_pg_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                           const uint8_t* actions, const float* advantages, const float* returns,
                           const float* old_prob, const int8_t* valids_or_null,
                           const int32_t* idx_or_null, const float* lr_mult,
                           const float* inv_count_or_null, int64_t batch, int32_t hid,
                           int32_t n_actions, int32_t kind, int32_t tie_rule, float clip_param,
                           float v_loss_coeff, float ent_loss_coeff, int32_t relu_mask_dh, float* dout, float* dh,
                           float* dw_head, float* db_head, float* loss4, void* workspace,
                           struct arl_fold_item* items3, const struct arl_dgrad_wt* wt_items_or_null, int32_t n_wt,
                           void* stream);

/* Phasic policy gradient (PPG, single-network variant): arl_pg_head_loss_parts' sibling for PPG's two phases
 * (csrc/ppg.hip; both entries run ONE kernel source and launcher, csrc/head_kernel_dev.h, and differ in the loss they
 * hand it).  The forward is the sibling's: o_k = sum_j h[b][j] W[k][j] + b_head[k] (lanes split j, lane l sums
 * j = l, l + 64, ... ascending, butterfly sum over the wave), p = softmax(o[0..A)) (max over k ascending, z = sum_k
 * exp(o_k - max) k ascending, p_k = exp(o_k - max) / z), V = o[A], TINY = 1e-8.  Rows of actions / advantages /
 * returns / old_prob are selected by idx_or_null (NULL = identity); inv_n = inv_count_or_null ? inv_count[0] :
 * 1 / (float) batch.  There are no valids.
 *
 * phase ARL_PPG_POLICY (0): pi_loss, v_loss, ent_loss, dout, dw_head, db_head are those of arl_pg_head_loss_parts
 *   kind 1 (PPO) with the same three tie_rules and clip = clip_param * lr_mult[0], expression for expression.  The
 *   value gradient is stopped at the last shared layer:
 *       dh[b][c] = sum_{k < A} dout[b][k] W[k][c]                     (k ascending; the value row k = A is left out)
 *   while dw_head = sum_b dout[b] x h[b] and db_head = sum_b dout[b] keep all A + 1 rows: the value loss trains W[A]
 *   and b_head[A] and nothing else.  loss4 = (pi, v, ent, (pi + v) + ent).  beta_clone is ignored.
 * phase ARL_PPG_AUX (1): actions, advantages, lr_mult may be NULL; clip_param, ent_loss_coeff, tie_rule are ignored;
 *   old_prob f32[n_rows][A] is read whole.  With w = inv_n, c = beta_clone * w, old = old_prob[row]:
 *       kl_b   = sum_k old_k * (log(old_k + TINY) - log(p_k + TINY))               (Categorical.kl_sym; k ascending)
 *       clone  = sum_b c * kl_b            v_loss = sum_b (v_loss_coeff * w * (V_b - R_b)) * (V_b - R_b)
 *       q_k    = old_k * p_k / (p_k + TINY),  S = sum_k q_k                        (k ascending)
 *       dout[b][j] = c * (p_j * S - q_j), j < A          dout[b][A] = 2 * v_loss_coeff * w * (V_b - R_b)
 *       dh[b][c] = sum_{k <= A} dout[b][k] W[k][c]                                 (k ascending)
 *   loss4 = (clone, v_loss, 0, (clone + v_loss) + 0).
 * Sums over b: wave w of workgroup g takes rows 4 g + w, + 4 * grid, ... in ascending order (grid = min(ceil(batch /
 * 4), 256)); a workgroup adds its four waves' sums in wave order; arl_fold_many adds the workgroups' partials in its
 * own fixed order.  The head weight gradient is summed in the launch itself while (A + 1) hid <= 3 072, else by the
 * separate row-split kernel, exactly as for the sibling.  No atomics anywhere: two launches on the same inputs give
 * the same bits.
 * relu_mask_dh != 0: dh[b][c] = 0 where !(h[b][c] > 0).
 *   out: dout f32[batch][A+1], dh f32[batch][hid]; dw_head f32[A+1][hid], db_head f32[A+1], loss4 f32[4] are described
 *        in items3[0..2] for arl_fold_many as arl_pg_head_loss_parts describes them (16-byte aligned)
 *   workspace >= arl_pg_head_workspace_bytes(), live until the fold has run
 * This entry does not write the arl_dgrad_wt weight copies: the backward pass launches arl_conv2d_dgrad_weights itself.
 * Limits (else ARL_E_RANGE): 1 <= n_actions <= 18, 1 <= hid <= 1024, 1 <= batch <= 2^31 - 1.  ARL_E_ARG: a NULL
 * mandatory pointer, a phase outside {0, 1}, in the policy phase a tie_rule outside its three values, or a coefficient
 * the phase reads that is not finite (policy: clip_param, v_loss_coeff, ent_loss_coeff; auxiliary: v_loss_coeff,
 * beta_clone).  A refused call launches nothing and writes nothing.                                               */
#define ARL_PPG_POLICY 0
#define ARL_PPG_AUX    1
int arl_ppg_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                            const uint8_t* actions, const float* advantages, const float* returns,
                            const float* old_prob, const int32_t* idx_or_null, const float* lr_mult,
                            const float* inv_count_or_null, int64_t batch, int32_t hid, int32_t n_actions,
                            int32_t phase, int32_t tie_rule, float clip_param, float v_loss_coeff,
                            float ent_loss_coeff, float beta_clone, int32_t relu_mask_dh, float* dout, float* dh,
                            float* dw_head, float* db_head, float* loss4, void* workspace,
                            struct arl_fold_item* items3, void* stream);

/* V-MPO (single-GPU, feed-forward, synchronous variant; csrc/vmpo.hip): the policy is regressed onto the better half of
 * a minibatch with weights softmax(A / eta), a trust region KL(old || pi) <= eps_alpha is held by a learned multiplier
 * alpha, and the temperature eta is learned from its own dual loss.  duals is a device f32[2] = (eta, alpha); both
 * kernels that need a dual read it on the device (the values move inside a captured graph).  TINY = 1e-8.
 *
 * arl_vmpo_weights: the top half of n advantages and its weights.  Position b = 0 .. n - 1 stands for row
 *   r(b) = idx_or_null ? idx[b] : b of `advantages` and of `psi` (idx must not repeat a row); A_b = advantages[r(b)].
 *       n_top    = (n + 1) / 2                                                          (integer division)
 *       key(a)   = bits(a) ^ (sign bit of a ? 0xFFFFFFFF : 0x80000000)                  (uint32; orders fp32 values, +0 above -0)
 *       selected = the n_top positions first in (key descending, b ascending)           (ties go to the lower position)
 *   The selection is exact: an integer radix select (four passes of 8 bits, most significant first, on an LDS histogram
 *   of integer atomics) finds the n_top-th largest key T and the number of keys equal to T that are selected; a prefix
 *   count over the positions in ascending order hands those places to the first ties.  What follows is float64 on the
 *   promoted fp32 inputs, eta = (double) duals[0], m = the largest advantage (always selected):
 *       e_b = exp((A_b - m) / eta) for selected b,   S = sum_b e_b,   psi_b = e_b / S,   SA = sum_b psi_b * A_b
 *       L   = m / eta + log(S / n_top)
 *       psi[r(b)]  = (float) psi_b for selected b, 0.f for every other position of the minibatch
 *       temp4      = ((float) (eta * eps_eta + eta * L), (float) ((eps_eta + L) - SA / eta), (float) L, (float) n_top)
 *   i.e. the temperature's dual loss, its derivative with respect to eta, the log mean exp(A / eta) of the selection
 *   and the selection's size; every output is rounded to fp32 once.  Sums over b: thread t of the one workgroup of
 *   1 024 adds its positions t, t + 1 024, ... in ascending order, a wave adds by halving shuffles (offsets 32 .. 1),
 *   the workgroup adds its 16 waves in wave order.  No float atomics: two launches on the same inputs give the same bits.
 *   Elements of psi that are no row of the minibatch are not written.  advantages must be finite and eta > 0 (not
 *   checked: the kernel reads them on the device).
 *   Limits: 1 <= n <= ARL_VMPO_MAX_ROWS (else ARL_E_RANGE); ARL_E_ARG: a NULL advantages, duals, psi or temp4, an
 *   eps_eta that is not finite.  A refused call launches nothing and writes nothing.
 *
 * arl_vmpo_head_loss_parts: arl_ppg_head_loss_parts' sibling (the same kernel source and launcher,
 *   csrc/head_kernel_dev.h; forward, row order of the sums, fold items, workspace and relu_mask_dh exactly as stated
 *   there).  Rows of actions / psi / returns / old_prob are selected by idx_or_null; psi is arl_vmpo_weights' output
 *   (already normalised over the minibatch: it takes no 1 / n); old_prob f32[n_rows][A] is read whole.  With
 *   w = inv_n, alpha = duals[1], a = actions[row], old = old_prob[row], c = alpha * w:
 *       pi_b   = -psi_b * log(p_a + TINY)
 *       kl_b   = sum_k old_k * (log(old_k + TINY) - log(p_k + TINY))                   (k ascending)
 *       q_k    = old_k * p_k / (p_k + TINY),  S = sum_k q_k                            (k ascending)
 *       g_a    = -psi_b / (p_a + TINY),  g_k = 0 elsewhere
 *       dout[b][j] = p_j * (g_j - g_a * p_a) + c * (p_j * S - q_j), j < A      dout[b][A] = 2 * v_loss_coeff * w * (V_b - R_b)
 *       dh[b][c] = sum_{k <= A} dout[b][k] W[k][c]                                     (k ascending: the value gradient
 *                                                                                       reaches the trunk)
 *   loss4 = (sum_b pi_b, sum_b (v_loss_coeff * w * (V_b - R_b)) * (V_b - R_b), sum_b w * kl_b, ([0] + [1]) + [2]): the
 *   KL is the plain mean, NOT scaled by alpha -- the dual step reads it -- so loss4[3] is not the Lagrangian the
 *   gradients belong to (that is [0] + [1] + alpha * [2]).  There is no entropy term, no ratio and no valids.
 *   This entry does not write the arl_dgrad_wt weight copies.
 *   Limits (else ARL_E_RANGE): 1 <= n_actions <= 18, 1 <= hid <= 1024, 1 <= batch <= 2^31 - 1.  ARL_E_ARG: a NULL pointer
 *   other than idx_or_null / inv_count_or_null, a v_loss_coeff that is not finite.  A refused call launches nothing.
 *
 * arl_vmpo_dual_step: one optimiser step on both duals in one launch of one workgroup, then the projection.
 *       g = (temp4[1], eps_alpha - loss4[2])                         (d temp_loss / d eta, d alpha (eps_alpha - KL) / d alpha)
 *       t = step_count[0] + 1,  lr = learning_rate * lr_mult[0],  adam: a_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)
 *       element i: the update of arl_opt_step with avg_factor 1 and no clipping, expression for expression
 *                  (slot0 = adam's m | rmsprop's accumulator, slot1 = adam's v; f32[2] each)
 *       duals[i] = max(duals[i], 1e-8);  step_count[0] = t
 *   Limits: method ARL_OPT_ADAM / ARL_OPT_RMSPROP, adam needs slot1, a finite eps_alpha, non-NULL pointers (ARL_E_ARG);
 *   beta1, beta2 in [0, 1) (rmsprop: rho in [0, 1]), epsilon >= 0, learning_rate >= 0 (ARL_E_RANGE).               */
#define ARL_VMPO_MAX_ROWS 65536
int arl_vmpo_weights(const float* advantages, const int32_t* idx_or_null, int64_t n, const float* duals,
                     double eps_eta, float* psi, float* temp4, void* stream);
int arl_vmpo_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                             const uint8_t* actions, const float* psi, const float* returns,
                             const float* old_prob, const int32_t* idx_or_null, const float* duals,
                             const float* inv_count_or_null, int64_t batch, int32_t hid, int32_t n_actions,
                             float v_loss_coeff, int32_t relu_mask_dh, float* dout, float* dh,
                             float* dw_head, float* db_head, float* loss4, void* workspace,
                             struct arl_fold_item* items3, void* stream);
int arl_vmpo_dual_step(float* duals, float* slot0, float* slot1_or_null, float* step_count,
                       const float* lr_mult, const float* temp4, const float* loss4, float eps_alpha,
                       int32_t method, float learning_rate, float beta1_or_rho, float beta2, float epsilon,
                       void* stream);

/* Random network distillation (RND; csrc/rnd.hip): the stages the exploration bonus adds around its two conv trunks
 * (which run on the contraction entry points below).  One value head, one reward stream.  float64 on the promoted
 * inputs, every output rounded once, no float atomics, no process-wide state; every shape is an argument, nothing
 * synchronises with the host.  A refused call launches nothing and writes nothing.
 *
 * The frame RND sees for transition (n, t) of an env-major rollout -- observations u8[n_env * horizon][C][H][W],
 * extra_observations u8[n_env][C][H][W], planes stacked oldest -> newest -- is the NEWEST plane of the NEXT observation:
 *       F(n, t) = observations[n * horizon + t + 1][C - 1]   if t + 1 < horizon,   else extra_observations[n][C - 1]
 * read in place (no copy is made).  Row r of the batch is (n, t) = (r / horizon, r % horizon).
 * Frame arguments, checked by arl_rnd_obs_stats and arl_rnd_obs_prepare: NULL observations / extra_observations
 * (ARL_E_ARG); n_env < 1, horizon outside 1 .. ARL_RND_MAX_HORIZON, n_env * horizon > ARL_RND_MAX_ROWS, channels outside
 * 1 .. 1024, h or w < 1, h * w > ARL_RND_MAX_PIXELS (ARL_E_RANGE).
 *
 * Chan's merge, as both running-moment entry points apply it to a state (na, mean, m2) and a batch (nb, mean_b, m2_b):
 *       w = nb / (na + nb);  delta = mean_b - mean;  mean' = mean + delta * w;
 *       m2' = (m2 + m2_b) + ((delta * delta) * na) * w;  count' = na + nb            (start from count = 0, mean = m2 = 0)
 *
 * arl_rnd_obs_stats: per pixel p, over the R = n_env * horizon frames of the batch,
 *       Sx = sum F[p], Sxx = sum F[p]^2 as uint64 integers -- exact, so neither the split of the rows across workgroups
 *       (ARL_RND_STATS_SPLITS of them: split z takes rows z, z + splits, ...) nor the order of the additions shows;
 *       mean_b = (double) Sx / R;   m2_b = (double) (R * Sxx - Sx * Sx) / R   (the numerator in uint64: R <= 2^24 keeps
 *       R * Sxx <= 2^48 * 65025 < 2^64 -- that is ARL_RND_MAX_ROWS -- and it is >= 0; a constant pixel gives exactly 0),
 *       then Chan's merge into (count[0], mean[p], m2[p]) with nb = R; count[0] is written once.
 *   count f64[1], mean and m2 f64[h * w], workspace >= arl_rnd_obs_stats_workspace_bytes(h, w) bytes (0 for sizes the
 *   entry point refuses), all 8-byte aligned (ARL_E_ALIGN); a NULL one: ARL_E_ARG.  Two launches.
 *
 * arl_rnd_obs_prepare: out f32[batch][h][w][4] (NHWC, 16-byte aligned), row b from batch row r = idx_or_null ? idx[b] : b:
 *       sd_p = sqrt(m2[p] / count[0] + 1e-8);   z = ((double) F(r)[p] - mean[p]) / sd_p;   z = max(z, -5), then min(z, 5)
 *       out[b][p] = ((float) z, 0, 0, 0)
 *   i.e. the four-channel padding the contraction kernels want for a one-plane input.  count[0] must be > 0 (it lives on
 *   the device and is not checked); idx values are not checked either.  1 <= batch <= ARL_RND_MAX_ROWS, and without idx
 *   batch <= n_env * horizon (ARL_E_RANGE); out not 16-byte, idx not 4-byte, count / mean / m2 not 8-byte aligned:
 *   ARL_E_ALIGN; a NULL count, mean, m2 or out: ARL_E_ARG.
 *
 * arl_rnd_error: pred, targ f32[batch][width].  One wave per row.  With d_e = (double) pred[b][e] - (double) targ[b][e]:
 *       lane l adds d_e * d_e over e = 4 (l + 64 k) + (0, 1, 2, 3), k = 0, 1, ... in that order; the wave adds its 64
 *       lanes by halving shuffles (offsets 32 .. 1);   err[b] = (float) (S / width)
 *   and with want_grad:
 *       dpred[b][e] = (float) ((2 * d_e) / ((double) width * (double) batch))
 *       loss[0]     = (float) (T / batch),  T = sum_b (double) err[b]: thread t of ONE workgroup of 1 024 adds b = t,
 *                     t + 1 024, ... in ascending order, a wave adds by halving shuffles, the 16 waves add in wave order
 *   (a second launch).  Without want_grad dpred and loss are not touched and may be NULL.
 *   width a multiple of 4 in 4 .. ARL_RND_MAX_WIDTH, 1 <= batch <= ARL_RND_MAX_ROWS (ARL_E_RANGE); pred, targ, dpred not
 *   16-byte, err, loss not 4-byte aligned (ARL_E_ALIGN); a NULL pred, targ, err, or dpred / loss with want_grad: ARL_E_ARG.
 *
 * arl_rnd_reward_mix: err, r_ext f32[n_env][horizon]; rho f64[n_env] and moments f64[3] = (count, mean, m2) are carried
 *   across calls (start from zeros).  One workgroup of 1 024, in this order:
 *       1. per env n, t ascending:  rho[n] = gamma_int * rho[n] + (double) err[n][t];  v[n][t] = rho[n]   (dones ignored:
 *          the bonus stream is not episodic)
 *       2. batch moments of the M = n_env * horizon values v_j, j = n * horizon + t:  mean_b = (sum_j v_j) / M,
 *          m2_b = sum_j (v_j - mean_b)^2; every sum: thread t adds j = t, t + 1 024, ... ascending, then as loss[0] above
 *       3. Chan's merge of (M, mean_b, m2_b) into moments -- BEFORE this batch is normalised
 *       4. sd = sqrt(m2 / count + 1e-8);  a = c_ext * (double) r_ext[j];  b = c_int * ((double) err[j] / sd);
 *          r_mix[j] = (float) (b == 0 ? a : a + b)        (so c_ext = 1, c_int = 0 and finite err return r_ext's bits)
 *       diag2 = ((float) ((sum_j (double) err[j]) / M), (float) sd)
 *   workspace: f64[n_env * horizon], 8-byte aligned like rho and moments; float pointers 4-byte (ARL_E_ALIGN).
 *   A single workgroup walks everything: n_env <= ARL_RND_MIX_MAX_ENVS (2^20), horizon <= ARL_RND_MAX_HORIZON, n_env *
 *   horizon <= ARL_RND_MIX_MAX_ROWS (2^22: 4 096 values per thread, 16 MiB of err -- past that the launch is no longer
 *   the few-KB-to-MB latency case it is written for) (ARL_E_RANGE).  ARL_E_ARG: a NULL pointer, gamma_int outside
 *   [0, 1] or not finite, c_ext or c_int not finite, r_mix equal to err or r_ext.                                     */
#define ARL_RND_MAX_ROWS     16777216
#define ARL_RND_MAX_PIXELS   16777216
#define ARL_RND_MAX_HORIZON  4096
#define ARL_RND_MAX_WIDTH    65536
#define ARL_RND_STATS_SPLITS 32
#define ARL_RND_MIX_MAX_ENVS 1048576
#define ARL_RND_MIX_MAX_ROWS 4194304
int64_t arl_rnd_obs_stats_workspace_bytes(int32_t h, int32_t w);
int arl_rnd_obs_stats(const uint8_t* observations, const uint8_t* extra_observations, int64_t n_env, int32_t horizon,
                      int32_t channels, int32_t h, int32_t w, double* count, double* mean, double* m2, void* workspace,
                      void* stream);
int arl_rnd_obs_prepare(const uint8_t* observations, const uint8_t* extra_observations, const int32_t* idx_or_null,
                        int64_t batch, int64_t n_env, int32_t horizon, int32_t channels, int32_t h, int32_t w,
                        const double* count, const double* mean, const double* m2, float* out, void* stream);
int arl_rnd_error(const float* pred, const float* targ, int64_t batch, int32_t width, int32_t want_grad, float* err,
                  float* dpred, float* loss, void* stream);
int arl_rnd_reward_mix(const float* err, const float* r_ext, int64_t n_env, int32_t horizon, double* rho, double* moments,
                       double gamma_int, double c_ext, double c_int, float* r_mix, float* diag2, void* workspace,
                       void* stream);

/* PopArt (adaptive value normalisation, single task; csrc/popart.hip): what an actor-critic whose value output is a
 * NORMALISED value n adds between its rollout and its optimiser step.  The unnormalised value of a state is sigma n + mu.
 * float64 on the promoted inputs, every output rounded once, no float atomics, no process-wide state; nothing
 * synchronises with the host.  A refused call launches nothing and writes nothing.
 *
 * stats f64[4] = (mu, nu, sigma, n_updates): first moment, second moment, the clamped standard deviation, the number of
 *   updates applied; lives on the device, carried across calls, starts as (0, 1, 1, 0); 8-byte aligned (ARL_E_ALIGN).
 *
 * arl_popart_denorm: value[i] = (float) (sigma * (double) value_n[i] + mu) for i < rows and last_value[k] likewise from
 *   last_n[k] for k < n_last -- one streaming launch over both arrays; the statistics are only read.
 *   1 <= rows <= ARL_POPART_MAX_ROWS, 1 <= n_last <= rows (ARL_E_RANGE); a NULL pointer, or an output that overlaps an
 *   input or the other output: ARL_E_ARG (the recorded values are another owner's buffer and are never written); float
 *   pointers not 4-byte aligned: ARL_E_ALIGN.
 *
 * arl_popart_step: returns f32[rows] (the regression targets G, unnormalised), advantages f32[rows] or NULL, valids
 *   i8[rows] or NULL (every row counts); w_value f32[hid] and b_value f32[1] are the value row and the value bias of the
 *   output layer (row A of W_head[(A + 1)][hid] starts A * hid floats in: 4-byte alignment is all that is asked).  One
 *   workgroup of 1 024, in this order:
 *       1. cnt = sum_i v_i, S1 = sum_i v_i G_i, S2 = sum_i v_i G_i G_i with v_i = (valids[i] != 0) and G_i promoted --
 *          rows with v_i = 0 are skipped, not multiplied, so what they hold does not matter; every sum: thread t adds
 *          i = t, t + 1 024, ... ascending, a wave adds by halving shuffles (offsets 32 .. 1), the 16 waves add in wave
 *          order;   m1 = S1 / cnt,  m2 = S2 / cnt
 *       2. if cnt > 0 and m1 and m2 are finite:
 *              mu' = (1 - beta) * mu + beta * m1;   nu' = (1 - beta) * nu + beta * m2;
 *              sigma' = min(max(sqrt(max(nu' - mu' * mu', 0)), sigma_min), sigma_max);   n_updates' = n_updates + 1
 *          else stats, w_value and b_value keep their bits, step 3 is skipped and step 4 runs with mu' = mu, sigma' = sigma
 *       3. ratio = sigma / sigma' (one division);   w_value[j] = (float) ((double) w_value[j] * ratio), j < hid;
 *          b_value[0] = (float) (((sigma * (double) b_value[0] + mu) - mu') / sigma')
 *          -- so sigma' n' + mu' = sigma n + mu for every hidden row, up to one float32 rounding of each weight
 *       4. returns[i] = (float) (((double) G_i - mu') / sigma');  advantages[i] = (float) ((double) advantages[i] / sigma');
 *          rows with v_i = 0 are written 0 in both
 *       diag2 = ((float) mu', (float) sigma')
 *   beta = 0 with stats (0, 1, 1, .) is the identity on every array (a -0.0 bias aside).  No debiasing of the moments.
 *   1 <= rows <= ARL_POPART_MAX_ROWS (2^22: 4 096 rows per thread -- past that a single workgroup is no longer the
 *   latency case this is written for), 1 <= hid <= ARL_POPART_MAX_HID (ARL_E_RANGE); ARL_E_ARG: a NULL returns, stats,
 *   w_value, b_value or diag2, beta outside [0, 1] or NaN, sigma_min or sigma_max not finite, sigma_min <= 0, sigma_min >
 *   sigma_max, advantages overlapping returns; float pointers not 4-byte, stats not 8-byte aligned: ARL_E_ALIGN.       */
#define ARL_POPART_MAX_ROWS 4194304
#define ARL_POPART_MAX_HID  65536
int arl_popart_denorm(const float* value_n, int64_t rows, const float* last_n, int64_t n_last, const double* stats,
                      float* value, float* last_value, void* stream);
int arl_popart_step(float* returns, float* advantages_or_null, const int8_t* valids_or_null, int64_t rows, double beta,
                    double sigma_min, double sigma_max, double* stats, float* w_value, float* b_value, int32_t hid,
                    float* diag2, void* stream);

/* ------------------------------------------------------------------------- *
 * The policy network's dense contractions on the matrix cores (fp32 MFMA)
 * ------------------------------------------------------------------------- */

/* Geometry of one convolution layer; a dense layer is in_h = in_w = kh = kw = 1,
 * in_c = fan_in, out_c = units.  in_c and out_c must be multiples of 4.        */
typedef struct arl_conv_geom {
    int64_t batch;
    int32_t in_h, in_w, in_c;     /* input  x  f32[batch][in_h][in_w][in_c]  (NHWC)     */
    int32_t out_c, kh, kw;        /* weight w  f32[out_c][kh][kw][in_c] (correlation)   */
    int32_t stride, pad_h, pad_w; /* output y  f32[batch][out_h][out_w][out_c],
                                     out_h = (in_h + 2 pad_h - kh) / stride + 1          */
    int32_t route;                /* how the fp32 contractions of this call are computed: ARL_CONV_ROUTE_*  */
} arl_conv_geom;

/* arl_conv_geom::route (the reference's floatX is float32: accel_rl/policies/pg/networks/pg_cnn.py:45-86 through
 * Theano).  Operands and results are fp32 on every route; only the way through the matrix cores differs:
 *   ARL_CONV_ROUTE_SPLIT9 (0, the default of a zero-initialised struct): each fp32 operand is split EXACTLY into three
 *      bf16 pieces (24 significand bits = 3 x 8) and all nine piece products -- each exact in fp32 -- are accumulated
 *      in fp32 by v_mfma_f32_32x32x16_bf16: every product term of the fp32 contraction enters the sum exactly, only
 *      the accumulation rounds;
 *   ARL_CONV_ROUTE_FP32   v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain (157 TF/s peak on gfx950);
 *   ARL_CONV_ROUTE_SPLIT6 as SPLIT9 without the three smallest piece products (each below 2^-24 of |x y|);
 *   ARL_CONV_ROUTE_BF16   NOT an fp32 contraction -- the labelled reduced-precision option: each fp32 operand is ROUNDED
 *      (to nearest even) to one bf16 value on its way into the matrix cores, one product per multiply, fp32
 *      accumulation; tensors in memory stay fp32.  8 significand bits per operand: results differ from the other
 *      routes by ~2^-9 relative per product; never a default, never selected by the library.
 * u8 observations are exact in one bf16 piece (three products on both split routes, one on BF16).  Layers with <= 16 output
 * columns and the generic (any channel count) kernels always take the fp32 chain -- except the first convolution from u8
 * rows with 16 filters of 8 x 8 (spec 0), which runs on the image-stationary bf16-split kernel with half its tile idle.  Deterministic on every route;
 * any other value: ARL_E_ARG.  The route is an argument of the call: the library keeps no mode.                     */
#define ARL_CONV_ROUTE_SPLIT9 0
#define ARL_CONV_ROUTE_FP32   1
#define ARL_CONV_ROUTE_SPLIT6 6
#define ARL_CONV_ROUTE_BF16   2

/* Scratch for the split reductions below (fixed; the caller allocates once). */
int64_t arl_conv_workspace_bytes(void);

/* One entry point per operation; an optional operand is an `_or_null` argument, and NULL there changes nothing about what
 * the others do (bit for bit and launch for launch).
 *
 * Rectifier masks as bits (y_bits_or_null, mask_bits_or_null below).  A data gradient uses one thing of every value of
 * its f32 mask: whether it is > 0.  For an activation tensor y f32[rows][C] with C % 32 == 0 (rows in the tensor's own NHWC
 * order) the mask as bits is u32[rows][C / 32]: bit c % 32 of word c / 32 = (y[row][c] > 0.f) as the device evaluates it on
 * the stored value (NaN and -0 give 0, as in the f32 comparison) -- 1/32 of the bytes.  ARL_E_ALIGN unless 4-byte aligned.
 * The reference has no counterpart: Theano keeps the rectifier's input for T.grad (pg_cnn.py:47-68).                    */

/* y = conv(x, w) + bias, then max(., 0) if relu.  Replaces the forward of Lasagne's
 * Conv2DLayer / DenseLayer as used by PgCnn (accel_rl/policies/pg/networks/pg_cnn.py:47-68,
 * policies/layers.py:22-41; the reference's flipped filters are stored pre-flipped).
 * Deterministic: fp32 MFMA accumulation in k order, split-K folded in a fixed order.
 * y_bits_or_null: the launch also writes y's mask as bits; y itself is written as ever.  Served on the bf16-split routes by
 *   the kernels of layers with 32 .. 64 output columns whose k-tiles hold one filter tap (in_c % 32 == 0: the learner's
 *   conv 2 and conv 3); ARL_E_RANGE -- nothing launched, never ignored -- for out_c % 32 != 0, a reduction that the call
 *   splits (the fold writes y; with item_or_null too), the fp32 route, wider or multi-tap layers and the generic kernels.
 * item_or_null: non-NULL leaves a split reduction unfolded and describes it, NULL folds here.  When the launch split its
 *   reduction the partial sums stay in `workspace` and *item describes them (part f32[splits][rows * out_c], total = rows
 *   * out_c; bias and rectifier NOT applied: they belong to whoever folds -- arl_env_step_served below does, per env,
 *   inside its launch); item->splits == 0: the launch did not split, y is final (bias and rectifier applied).  The
 *   workspace stays live until the consumer has run.                                                                  */
int arl_conv2d_fwd(const float* x, const float* w, const float* bias_or_null, float* y, uint32_t* y_bits_or_null,
                   const arl_conv_geom* geom, int32_t relu, void* workspace, arl_fold_item* item_or_null, void* stream);
/* How arl_conv2d_fwd walks this geometry's reduction (host-side, nothing launched): *splits = the number of
 * partial sums per output (1: not split) and *k_per_split = the reduction indices of one.  Two geometries of one layer
 * that differ only in `batch` give every row the same bits when both numbers agree and the route is one of the
 * bf16-split ones (ARL_CONV_ROUTE_SPLIT9 / _SPLIT6): their kernels issue the same piece products in the same k order
 * whatever the tile shape the launch's size picks, and the fold's order depends on the split count alone.  A caller
 * that wants to reuse rows computed at another batch size (the rollout's activations in the learner) asks here.
 * NULL pointers, a bad geometry or route: as arl_conv2d_fwd.                                                        */
int arl_conv2d_fwd_plan(const arl_conv_geom* geom, int32_t* splits, int32_t* k_per_split);

/* Convolution 1 read straight from the sampler's observations (no f32 copy of the input):
 * obs u8[obs_rows][in_c][in_h][in_w] (the layout of samples_buf.observations,
 * accel_rl/sampler/act_server/buffers.py:7-38), row b of the batch = obs[idx ? idx[b] : b]
 * (the minibatch indices of optimizers/util.py:8-18), x = float(byte) * scale
 * (atari_cnn_policy.py:88-91: the network input is obs * (1 / 255)).  Weights and their gradient are
 * f32[out_c][in_c][kh][kw] (correlation kernels).  geom->batch = rows of the batch; in_c any count >= 1.
 * Requires pad 0, stride % 4 == 0, in_w % 4 == 0, (in_h * in_w) % 4 == 0, kw in {4, 8, 16},
 * kh % (16 / kw) == 0, out_c % 4 == 0 and <= 32 (else ARL_E_RANGE: use arl_gather_scale_obs_nhwc +
 * arl_conv2d_fwd).  The sums run over the exact integer pixels, plane by plane, and `scale` multiplies the
 * finished sum once (a convolution is linear in its input: y = scale * conv(byte, w) + bias) -- equal to the
 * gather + scale route up to f32 round-off, not bit for bit.
 * y_bits_or_null: as arl_conv2d_fwd's.  Served on the bf16-split routes with 32 filters (the image-stationary kernel, or
 *   the tap-gathering split kernel where that one does not run); ARL_E_RANGE, nothing launched, anywhere else.  */
int arl_conv2d_u8_fwd(const uint8_t* obs, int64_t obs_rows, const int32_t* idx_or_null, float scale,
                      const float* w, const float* bias_or_null, float* y, uint32_t* y_bits_or_null,
                      const arl_conv_geom* geom, int32_t relu, void* stream);

/* dx = gradient of the layer input given dy (every element of dx is written).
 * If mask is given (same shape as dx): dx = 0 where mask <= 0 -- the rectifier
 * backward of the previous layer.  Requires kh % stride == 0 and kw % stride == 0.
 * Replaces the T.grad of the same layers (optimizers/single/ppo_optimizer.py:38-40).
 * wt_or_null: arl_conv2d_dgrad_weights' copy of w (below).
 * mask_bits_or_null: the mask of mask_or_null as bits, from a forward call's y_bits on the same tensor.  It comes on top of
 *   mask_or_null (ARL_E_ARG without it): the bf16-split launches of 17 .. 64 input channels on the k-contiguous weight
 *   copy (wt) and the shared launch of arl_conv2d_bwd_pair test the bit and never read the floats; every other launch
 *   (fp32 route, no wt, 16-wide tiles, generic kernels, the split reduction's fold) compares the floats as before.  dx
 *   is the same bits either way.  ARL_E_RANGE for in_c % 32 != 0.
 * job (optional): an optimiser job (arl_corun_job, below) that this call's launch may carry in extra workgroups;
 *   *job_taken = 1 if it did (only the scalar-addressed data-gradient launches of layers with > 16 input channels
 *   can), else 0 and the caller runs the job itself (arl_corun_job_run). */
struct arl_corun_job;
int arl_conv2d_bwd_data(const float* dy, const float* w, const float* wt_or_null, const float* mask_or_null,
                        const uint32_t* mask_bits_or_null, float* dx, const arl_conv_geom* geom,
                        const struct arl_corun_job* job_or_null, int32_t* job_taken_or_null, void* stream);

/* The data gradient's own copy of a layer's weights: per input-pixel parity class (ph, pw) of the stride a matrix
 * wt[ph * stride + pw][in_c][(ty * kw / stride + tx) * out_c + k] = w[k][i0 + stride ty][j0 + stride tx][c], (i0, j0) =
 * ((ph + pad_h) % stride, (pw + pad_w) % stride) -- the reduction index of dx = conv^T(dy, w) contiguous, as a forward pass
 * finds its weights.  Same size as w; one launch converts up to ARL_DGRAD_WT_MAX layers (after every parameter update,
 * before the backward pass that reads them).  Given as wt_or_null to arl_conv2d_bwd_data / arl_conv2d_bwd_pair, the
 * bf16-split kernels of 17 .. 64 input channels read it instead of w: the same piece products in the same order
 * (bit-identical results), a third less LDS and loader work per k-tile.  The reference has no counterpart: Theano's
 * conv gradient picks its own layout inside cuDNN (T.grad of pg_cnn.py:47-68, optimizers/single/ppo_optimizer.py:38-40). */
typedef struct arl_dgrad_wt {
    const float* w;             /* f32[out_c][kh][kw][in_c]                                                */
    float* wt;                  /* f32[out_c * kh * kw * in_c], 16-byte aligned, not aliasing w            */
    const arl_conv_geom* geom;  /* kh, kw divisible by stride, stride <= 2                                 */
} arl_dgrad_wt;
#define ARL_DGRAD_WT_MAX 4
int arl_conv2d_dgrad_weights(const arl_dgrad_wt* items, int32_t n, void* stream);

/* dw f32[out_c][kh][kw][in_c] = gradient of the layer weights given dy and the layer
 * input x; the reduction over batch x out_h x out_w is split across workgroups and
 * folded in a fixed order (no atomics).                                           */
int arl_conv2d_bwd_weight(const float* dy, const float* x, float* dw, const arl_conv_geom* geom,
                          void* workspace, void* stream);

/* A weight gradient described instead of launched (plan_or_null below; run by arl_conv2d_bwd_weight_group). */
typedef struct arl_wgrad_plan { int64_t opaque[32]; } arl_wgrad_plan;

/* Deferred-fold variant (arl_fold_item above; arl_fold_many folds).
 * dbias (optional): the kernel also leaves per-split column sums of dy (the bias gradient of a layer
 *   whose dy is already masked by its rectifier) behind the weight partials and describes their fold in
 *   *bias_item; bias_item->splits == -1 means "not produced" (the generic kernels ran): use
 *   arl_relu_bwd_bias_grad / _parts instead.
 * plan_or_null: non-NULL plans only -- the call validates, plans the row split and fills the fold item(s) exactly as
 *   with NULL (same workspace, same split count, same partial layout, same bias partials), describes its launch in
 *   *plan and launches nothing; `stream` is not used. */
int arl_conv2d_bwd_weight_parts(const float* dy, const float* x, float* dw, const arl_conv_geom* geom,
                                void* workspace, int64_t workspace_bytes, arl_fold_item* item,
                                float* dbias_or_null, arl_fold_item* bias_item_or_null, arl_wgrad_plan* plan_or_null,
                                void* stream);
/* The same for arl_conv2d_u8_fwd's layer. */
int arl_conv2d_u8_bwd_weight_parts(const float* dy, const uint8_t* obs, int64_t obs_rows,
                                   const int32_t* idx_or_null, float scale, float* dw,
                                   const arl_conv_geom* geom, void* workspace, int64_t workspace_bytes,
                                   arl_fold_item* item, float* dbias_or_null,
                                   arl_fold_item* bias_item_or_null, arl_wgrad_plan* plan_or_null, void* stream);
int arl_fold_many(const arl_fold_item* items, int32_t n, void* stream);

/* A layer's data gradient and weight gradient (deferred fold) as ONE launch: the two are independent
 * and both read dy, so their workgroups share a grid -- one ramp-up and one tail instead of two, and
 * the second problem's workgroups fill the CUs the first one's last wave leaves idle.  Same results as
 * arl_conv2d_bwd_data + arl_conv2d_bwd_weight_parts (which it falls back to when either side is not
 * on the scalar-addressed fast path); wt_or_null, mask_bits_or_null, the job and dbias as there.
 * plan_or_null: non-NULL leaves the weight gradient of a layer that does not pair to the group -- the data gradient is
 *   launched now (and carries the job), the weight gradient is planned into *plan; a layer that pairs runs its shared
 *   launch now and leaves *plan empty (the group skips it). */
int arl_conv2d_bwd_pair(const float* dy, const float* w, const float* wt_or_null, const float* mask_or_null,
                        const uint32_t* mask_bits_or_null, float* dx, const float* x, float* dw,
                        const arl_conv_geom* geom, void* workspace, int64_t workspace_bytes, arl_fold_item* item,
                        float* dbias_or_null, arl_fold_item* bias_item_or_null,
                        const struct arl_corun_job* job_or_null, int32_t* job_taken_or_null,
                        arl_wgrad_plan* plan_or_null, void* stream);

/* Several layers' weight gradients as ONE launch.  The weight gradients of a backward pass do not depend on one another
 * (each reads its own layer's dy and input), so the caller walks the data gradients first and has every weight gradient
 * planned (plan_or_null above, a caller-owned arl_wgrad_plan per layer).  arl_conv2d_bwd_weight_group then
 * runs up to ARL_WGRAD_GROUP_MAX plans: those on a bf16-split route whose kernel is one of the 64-filter f32 tile or the
 * two u8 tiles share one grid -- every workgroup finds its layer from its block index and does what its layer's own
 * launch would have had it do, writing where it would have written (bit-identical partials; no synchronisation between
 * workgroups) -- one ramp and one tail instead of three, and the L1-bound u8 workgroups resident beside matrix-bound
 * ones.  Every other plan (fp32 route, generic kernels, <= 16 filters, other tiles, a trace buffer set) is launched on
 * its own first, as the planning call would have with plan_or_null = NULL; so is a single eligible plan.  The plans'
 * buffers must stay untouched between the planning call and the group's launch.
 * Replaces the same T.grad nodes as arl_conv2d_bwd_weight (optimizers/single/ppo_optimizer.py:38-40).               */
#define ARL_WGRAD_GROUP_MAX 4
int arl_conv2d_bwd_weight_group(const arl_wgrad_plan* plans, int32_t n, void* stream);

/* ------------------------------------------------------------------------- *
 * One agent step of action serving in ONE launch
 * ------------------------------------------------------------------------- */

/* The policy's output layers as arl_env_step_served evaluates them for every env (row e of each array = env e). */
typedef struct arl_serve_head {
    arl_fold_item hidden;       /* the last hidden layer as arl_conv2d_fwd's item has it:   total = n_env * hid;
                                 * splits > 0: part f32[splits][n_env][hid] partial sums (folded in arl_fold_many's order);
                                 * splits == 0: part f32[n_env][hid] finished activations.  `out` is not used.          */
    const float* hidden_bias;   /* f32[hid] or NULL: added after the fold (splits > 0 only)                             */
    int32_t hidden_relu;        /* != 0: max(., 0) after the bias (splits > 0 only)                                     */
    int32_t hid;                /* multiple of 4, <= 1024                                                               */
    const float* w_head;        /* f32[n_actions + 1][hid], rows 0..A-1 pi, row A value (arl_pg_head_infer's layout)    */
    const float* b_head;        /* f32[n_actions + 1]                                                                   */
    float* hidden_out;          /* f32[n_env][hid], 16-byte aligned, or NULL: where the launch leaves the last hidden
                                 * layer as its heads read it (folded, bias and rectifier applied) -- with split partials
                                 * that row exists nowhere else.  NULL: nothing is stored, the launch is what it was.   */
} arl_serve_head;

/* The first convolution of the NEXT observation, evaluated from LDS right after the env step has built it
 * (arl_conv2d_u8_fwd's arithmetic; geometries: arl_serve_conv1_supported).                                            */
typedef struct arl_serve_conv1 {
    const arl_conv_geom* geom;  /* batch = n_env, in_c = n_stack, 104 x 80 input, 32 or 16 filters of 8 x 8, no padding*/
    const float* w;             /* f32[out_c][n_stack][8][8]                                                           */
    const float* bias;          /* f32[out_c] or NULL                                                                  */
    float* y;                   /* f32[n_env][out_h][out_w][out_c]                                                     */
    float scale;                /* pixel scale (1 / 255), applied to the finished sums                                 */
    int32_t relu;
} arl_serve_conv1;

/* 1 if arl_env_step_served can take this first layer (else: conv1_or_null = NULL and arl_conv2d_u8_fwd afterwards). */
int arl_serve_conv1_supported(const arl_game* game, const arl_conv_geom* geom);

/* arl_rollout_begin and arl_conv2d_u8_fwd of the rows it copies as ONE launch: observations[env * horizon + 0] =
 * step_obs[env] (overlap/worker.py:30-32), st->done_count[0] = 0, and conv1->y = the first convolution of those rows
 * (pg_cnn.py:47-52) -- the image passes through the kernel's registers once.  Geometries: arl_serve_conv1_supported.  */
int arl_rollout_begin_conv1(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                            const arl_serve_conv1* conv1, void* stream);

/* One (step, all envs) turn of serve_actions with everything per-env in one launch (one workgroup per env): fold, bias
 * and rectifier of the last hidden layer's split partials, the policy and value heads + softmax (arl_pg_head_infer),
 * weighted_sample_n, the env step (arl_env_step with mid_batch_reset != 0, single_write != 0, every env stepping) and,
 * with conv1, the first convolution of the observation the step has just produced (row e of conv1->y = env e; it
 * belongs to step + 1, or to the bootstrap observation after the batch's last step).  prob and value are written
 * straight to ro->prob / ro->value rows env * horizon + step.  Results are bit for bit those of the separate calls.
 * Replaces accel_rl/sampler/act_server/alternating/overlap/sampler.py:120-151 (serve_actions), the output layers of
 * _f_prob_value (policies/pg/atari_cnn_policy.py:63-67, pg/networks/pg_cnn.py:57-86), rllab/misc/special.py:22-27,
 * overlap/worker.py:37-59, envs/atari_env.py:65-78,93-100,151-191 and pg_cnn.py:47-52 for the next observation.
 * Needs st->next_reset, max_path_length >= 1, n_stack <= 4, 16-byte aligned observations / step_obs.
 * Limits (anything else is refused, nothing launched): head->hid a multiple of 4 and <= 1024; n_actions <=
 * ARL_MAX_ACTIONS (18); with split partials the fold's scratch zgn * hid * 4 bytes <= 64 KiB, where zgn = 16 below the
 * wide fold's threshold (128 splits) and 64 from it on -- i.e. any hid up to 1024 below the threshold, hid <= 256 from
 * it on; head->hidden.total == n_env * hid, splits >= 0, part and hidden_bias 16-byte aligned.  Any n_env >= 1 and any
 * envs_per_stream >= 1 (streams longer than n_env and a shorter last stream included).                              */
int arl_env_step_served(const arl_game* game, const arl_env_state* st, const arl_rollout* ro,
                        const arl_serve_head* head, const arl_serve_conv1* conv1_or_null,
                        const double* uniforms, int32_t step, double max_path_length, double discount,
                        int32_t max_start_noops, void* stream);

/* ------------------------------------------------------------------------- *
 * Replay memory of the DQN family
 * ------------------------------------------------------------------------- */

#define ARL_REPLAY_MAX_HORIZON 16

/* Frame-dedup replay storage for all environments, struct-of-arrays in HBM.
 * Replaces FrameReplayBuffer + one EnvBuffer per environment,
 * accel_rl/algos/dqn/replay_buffers/frame.py:23-119.  Per environment `size`
 * states; every frame is stored once in a ring of size + n_stack - 1 slots.
 * Both entry points refuse (ARL_E_RANGE, nothing launched) n_stack < 2, frame_bytes not a multiple of 16,
 * reward_horizon outside 1 .. min(ARL_REPLAY_MAX_HORIZON, size), and size < n_stack - 1 (the mirror of the
 * ring's tail would overlap itself, and no state of such a store could be sampled). */
typedef struct arl_replay {
    int64_t  n_env;
    int32_t  size;            /* states per environment (env_replay_size, frame.py:44) */
    int32_t  n_stack;         /* frames per observation (num_img_obs), >= 2            */
    int32_t  frame_bytes;     /* bytes of one frame, multiple of 16 (104*80 = 8320)    */
    int32_t  reward_horizon;  /* n of the n-step return                                */
    uint8_t* frames;          /* u8[n_env][size + n_stack - 1][frame_bytes]            */
    uint8_t* n_blanks;        /* u8[n_env][size + n_stack - 1] blank frames after a reset */
    uint8_t* acts;            /* u8[n_env][size]                                       */
    uint8_t* terminals;       /* u8[n_env][size] (0/1)                                 */
    float*   rewards;         /* f32[n_env][size]                                      */
    float*   returns;         /* f32[n_env][size] n-step discounted return             */
} arl_replay;

/* One sampler batch into the ring at state index idx: newest frame of every step,
 * actions / rewards / dones, blank-history marks after terminals, and the n-step
 * returns of the `horizon` states that now have all their rewards, with a terminal
 * inside the window propagated back.  Replaces append_data / write_samples,
 * frame.py:57-60,121-166.  Sampler layout, env-major: observations
 * u8[n_env*horizon][n_stack][frame_bytes], actions u8, rewards f32, dones u8.
 * promo as for the scans (the reference accumulates python-float x float32). */
int arl_replay_append(const arl_replay* rb, const uint8_t* observations, const uint8_t* actions,
                      const float* rewards, const uint8_t* dones, int32_t horizon, int32_t idx,
                      double discount, int32_t promo, void* stream);

/* Batch extraction: obs / next_obs (reward_horizon states later) as stacked u8 frames with
 * the post-reset blank frames zeroed, plus actions, n-step returns, terminals.
 * Replaces extract_batch / extract_observations, frame.py:69-90. */
int arl_replay_extract(const arl_replay* rb, const int32_t* env_idxs, const int32_t* step_idxs,
                       int64_t batch, uint8_t* obs, uint8_t* next_obs, uint8_t* actions,
                       float* returns, uint8_t* terminals, void* stream);

/* Batch extraction with DrQ's random shift (Kostrikov, Yarats, Fergus 2020; the reference has none): every observation
 * is padded by `pad` pixels with its own border and cropped back at a drawn offset, m_obs shifted views of obs and
 * k_next of next_obs per sample, in the one gather that reads the frames.
 *   obs u8[m_obs * batch][n_stack][frame_h][frame_w], next_obs u8[k_next * batch][n_stack][frame_h][frame_w], both
 *   view-major: view v of sample j is row v * batch + j (m_obs = k_next = 1: arl_replay_extract's layout);
 *   actions, returns, terminals [batch], exactly as arl_replay_extract writes them.
 * The source observation src is what arl_replay_extract produces for (env, step) -- (env, (step + reward_horizon) mod
 * size) for the next views -- its leading n_blanks frames zeroed.  Views are numbered v = 0 .. m_obs - 1 (obs) and
 * m_obs .. m_obs + k_next - 1 (next_obs); each draws ONE offset pair, shared by the n_stack frames of the stack:
 *   words = Philox4x32-10(key = ((uint32) seed, ARL_AUG_PHILOX_STREAM),
 *                         counter = ((uint32) j, (uint32) v, (uint32) call, (uint32)(call >> 32)))
 *   dx = (int)(((uint64) words[0] * (2 pad + 1)) >> 32) - pad;  dy likewise from words[1]      (both in -pad .. pad)
 *   out[f][y][x] = src[f][clamp(y + dy, 0, frame_h - 1)][clamp(x + dx, 0, frame_w - 1)]
 * which is an edge-replicating pad by `pad` followed by a crop at (pad + dy, pad + dx).  Zeroing a blank frame commutes
 * with the shift: it stays all zero.  pad == 0 performs no draw and its outputs equal arl_replay_extract's bit for bit.
 * seed and call are passed by value: extraction is an eager launch outside the captured update graph (the graph only
 * reads its static outputs), so no device-side generator state is needed; the caller advances `call` per extraction.
 * Integer-exact, plain vector stores, no atomics: equal (seed, call) give equal outputs.
 * Refused before any HIP call, nothing written: a NULL pointer (ARL_E_ARG); batch < 1 or >= 2^31, frame_h * frame_w !=
 * rb->frame_bytes, frame_w % 4 != 0, pad outside 0 .. 64, m_obs or k_next outside 1 .. 8, (m_obs + k_next) * batch >=
 * 2^31, and -- frames are staged through 16 KiB of LDS in tiles of whole rows -- frame_bytes > 16384 with
 * frame_w > 4088 (ARL_E_RANGE); obs or next_obs not 16-byte aligned (ARL_E_ALIGN).
 * Grid (batch, m_obs + k_next), one 256-thread workgroup per stacked view.                                          */
#define ARL_AUG_PHILOX_STREAM 0xA5D3F1C7u   /* second key word; >= 2^31 and != ARL_IQN_PHILOX_STREAM                  */
int arl_replay_extract_shift(const arl_replay* rb, const int32_t* env_idxs, const int32_t* step_idxs, int64_t batch,
                             int32_t frame_h, int32_t frame_w, int32_t pad, int32_t m_obs, int32_t k_next,
                             int64_t seed, int64_t call, uint8_t* obs, uint8_t* next_obs, uint8_t* actions,
                             float* returns, uint8_t* terminals, void* stream);

/* Parted sum tree of prioritized replay, f64[2^levels - 1], root at 0, children 2i+1 / 2i+2
 * (accel_rl/algos/dqn/replay_buffers/sum_tree.py:12-98).
 * find:   descend by prefix mass, uniforms in [0,1] scaled by the root       (:88-98)
 * add:    np.add.at along every leaf-to-root path; several updates of one node are
 *         applied in INPUT order, so the f64 rounding equals the reference's (:54-57)
 * gather: out[i] = scale * tree[idxs[i]]                                      (:65,:83) */
int arl_sumtree_find(const double* tree, int32_t levels, const double* uniforms, int64_t n,
                     int32_t* tree_idxs, void* stream);
int arl_sumtree_add(double* tree, int32_t levels, const int32_t* tree_idxs, const double* diffs,
                    int64_t n, void* stream);
int arl_sumtree_gather(const double* tree, const int32_t* tree_idxs, int64_t n, double scale,
                       double* out, void* stream);

/* The device half of PartedSumTree.sample_n (sum_tree.py:77-86): find() for m uniforms, sorted distinct
 * leaves, the n smallest kept with their probabilities and (part, step) = divmod(leaf, part_size);
 * n_unique[0] = number of distinct leaves found (< n: the reference would draw more -- the caller tops
 * up through arl_sumtree_find as before; output slots past the distinct leaves repeat the first one, so
 * consumers already queued stay in bounds).  1 <= n <= m <= 4096.                                 */
int arl_sumtree_sample(const double* tree, int32_t levels, const double* uniforms, int32_t m, int32_t n,
                       int32_t part_size, int32_t* tree_idxs, int32_t* env_idxs, int32_t* step_idxs,
                       double* probs, int32_t* n_unique, void* stream);

/* The same launch with the batch's importance-sampling weights (arl_is_weights on the n probabilities: prioritized.py:33-35)
 * and a host hand-off without a copy: uniforms may live in page-locked host memory (read once each), and
 * notify_or_null (page-locked, 8-byte aligned) receives (ticket << 32) | n_unique when everything above is written --
 * the one integer sample_n's caller waits for (sum_tree.py:80: `while len(tree_idxs) < n`) arrives by a store the host
 * polls instead of a memcpy node and an event.  is_weights_or_null f32[n] (slots past the distinct leaves: 0).       */
int arl_sumtree_sample_batch(const double* tree, int32_t levels, const double* uniforms, int32_t m, int32_t n,
                             int32_t part_size, int32_t* tree_idxs, int32_t* env_idxs, int32_t* step_idxs,
                             double* probs, int32_t* n_unique, double beta, float* is_weights_or_null,
                             int64_t* notify_or_null, int32_t ticket, void* stream);

/* update_batch_priorities on the device in ONE launch: arl_priority_diffs (f32 priorities ** alpha - the probabilities
 * sampled before) feeding arl_sumtree_add (np.add.at per level in input order); prioritized.py:37-38,
 * sum_tree.py:50-57,74-75.                                                                                          */
int arl_sumtree_update_pow(double* tree, int32_t levels, const int32_t* tree_idxs, const float* priorities,
                           const double* last_probs, double alpha, int64_t n, void* stream);

/* Importance-sampling weights of PrioritizedReplayBuffer.sample_batch (prioritized.py:33-35):
 * out[i] = f32( (1 / probs[i]) ** beta / max_j (1 / probs[j]) ** beta ), arithmetic in f64.        */
int arl_is_weights(const double* probs, int64_t n, double beta, float* out, void* stream);

/* diffs[i] = f64( f32(priorities[i] ** alpha) ) - last_probs[i]: the argument update_last_samples hands to
 * reconstruct (prioritized.py:37-38, sum_tree.py:74-75); follow with arl_sumtree_add.                */
int arl_priority_diffs(const float* priorities, const double* last_probs, int64_t n, double alpha,
                       double* diffs, void* stream);

/* ------------------------------------------------------------------------- *
 * Categorical DQN output stage
 * ------------------------------------------------------------------------- */

/* Action serving: per-action softmax over atoms, Q_a = sum_i p_ai z_i, greedy action = first
 * maximum; where override[b] >= 0 that action is taken instead (the epsilon-greedy draw, made
 * on the host RNG as the reference does).  The chosen action is written as a one-hot row so the
 * sampler's categorical kernel selects exactly it.  Replaces AtariCatDqnPolicy.get_actions /
 * actions_sym, accel_rl/policies/dqn/atari_cat_dqn_policy.py:84-126 (+ catdqn_cnn.py:94-99).
 *   logits f32[batch][n_actions][atom_stride], atom_stride % 4 == 0 >= n_atoms <= 64;
 *   z f32[n_atoms]; onehot f32[batch][n_actions]; greedy u8[batch] or NULL
 * dueling != 0 (DuelingMergeLayer, policies/dqn/layers/dueling_merge_layer.py:32-35, catdqn_cnn.py:77-93):
 *   logits f32[batch][n_actions + 1][atom_stride], advantage rows then ONE value row;
 *   logit(a, i) = val_i + (adv_ai - mean_a adv_ai) before the softmax.                    */
int arl_catdqn_act(const float* logits, const float* z, const int32_t* override_or_null, int64_t batch,
                   int32_t n_actions, int32_t n_atoms, int32_t atom_stride, int32_t dueling, float* onehot,
                   uint8_t* greedy_or_null, void* stream);

/* Loss of CategoricalDQN.build_loss, accel_rl/algos/dqn/cat_dqn.py:40-109: next action greedy
 * under the target net (or the policy net: double DQN), its atom probabilities under the target
 * net projected from the support shifted by the n-step return (clipped to [v_min, v_max], zeroed
 * gamma^n z where terminal) onto the base support; cross-entropy against clip(pred, 1e-6, 1),
 * importance-weighted mean; priorities = clip(KL, 1e-6, 1e6).
 *   out: dlogits f32[batch][n_actions][atom_stride] (d mean-loss / d pred_logits),
 *        loss_rows f32[batch] (their sum is the loss), kl f32[batch]
 * dueling != 0: all three logit blocks and dlogits are [n_actions + 1][atom_stride] as above;
 *   dlogits is the gradient w.r.t. the advantage rows and the value row (through the merge). */
int arl_catdqn_loss(const float* pred_logits, const float* tgt_next_logits, const float* pol_next_logits_or_null,
                    const float* z, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                    const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n_atoms,
                    int32_t atom_stride, int32_t dueling, float v_min, float v_max, float gamma_n,
                    float* dlogits, float* loss_rows, float* kl, void* stream);

/* The same loss reading its three logit blocks as the output layer's SPLIT PARTIAL SUMS (arl_conv2d_fwd's item on the
 * "action_atoms" dense layer, catdqn_cnn.py:69-76): at the reference's minibatch of 32 (accel_rl/algos/dqn/dqn.py:18) an
 * update is a chain of launch latencies, and the two launches that only fold the output layers' partials are taken
 * over by the loss kernel -- logit = (the partials summed in arl_fold_many's order) + bias, operation for operation, so
 * the results are arl_catdqn_loss's on the folded logits bit for bit.
 *   part          f32: this block's row 0 inside split 0 (the online pass over [obs; next_obs] hands `pred` its first
 *                 batch rows and `pol_next` the rows from batch on, same split_stride)
 *   split_stride  floats between consecutive splits (arl_fold_item.total of the forward launch)
 *   splits        1 .. 127 (arl_fold_item.splits; a launch that did not split: 1, with part = its finished output and
 *                 bias_or_null = NULL)
 *   bias_or_null  f32[(n_actions (+ 1)) * atom_stride]: the output layer's bias, added after the sum                  */
typedef struct arl_logit_src {
    const float* part;
    const float* bias_or_null;
    int64_t split_stride;
    int32_t splits;
    int32_t reserved;
} arl_logit_src;
int arl_catdqn_loss_parts(const arl_logit_src* pred, const arl_logit_src* tgt_next, const arl_logit_src* pol_next_or_null,
                          const float* z, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                          const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n_atoms,
                          int32_t atom_stride, int32_t dueling, float v_min, float v_max, float gamma_n,
                          float* dlogits, float* loss_rows, float* kl, const struct arl_dgrad_wt* wt_items_or_null,
                          int32_t n_wt, void* stream);
/* (wt_items_or_null / n_wt: as in arl_pg_head_loss_parts -- the launch also writes these layers' k-contiguous weight copies
 *  for the backward pass that follows, in extra workgroups.) */

/* ------------------------------------------------------------------------- *
 * Quantile-regression DQN output stage
 * ------------------------------------------------------------------------- */

/* QR-DQN (Dabney et al. 2018; the reference has none): the network predicts N = n_quantiles quantile locations per
 * action -- no fixed support, no projection.
 *   theta f32[batch][n_actions][q_stride], lane i of a wave = quantile i; the padding columns are ignored
 *   dueling != 0: theta f32[batch][n_actions + 1][q_stride], advantage rows then ONE value row, merged as the
 *   categorical head's: theta(a, i) = val_i + (adv_ai - mean_a adv_ai)
 * Limits (else ARL_E_RANGE, nothing launched, no output written): 1 <= batch < 2^31, 1 <= n_actions <= 64,
 *   2 <= n_quantiles <= 64, n_quantiles <= q_stride <= 2^20, q_stride % 4 == 0.  A NULL mandatory pointer: ARL_E_ARG.
 *
 * Action serving: Q_a = (sum_i theta(a, i)) / n_quantiles in fp32 (the 64 lanes summed as a butterfly: lane ^ 32, ^ 16,
 * ... ^ 1), greedy action = FIRST maximum (two identical rows tie to the lower index); override, the one-hot row and
 * `greedy` exactly as in the categorical action entry point above.
 *   onehot f32[batch][n_actions]; greedy u8[batch] or NULL                                                        */
int arl_qrdqn_act(const float* theta, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                  int32_t n_quantiles, int32_t q_stride, int32_t dueling, float* onehot, uint8_t* greedy_or_null,
                  void* stream);

/* Pairwise quantile-Huber loss with its gradient.  Per sample b, N = n_quantiles, w_b = (is_weight_b or 1) / batch,
 * tau_i = (i + 0.5) / N, keep = 1 - terminal_b:
 *   a*     = first maximum over a of Q_a (as above) under pol_next if given (double DQN), else under tgt_next
 *   T_j    = returns_b + keep * (gamma_n * theta_tgt(a*, j))                      (fp32, in this order)
 *   u_ij   = T_j - theta_pred(actions_b, i);  [u<0] = 1 for u < 0, else 0 (u == 0 counts as not negative)
 *   kappa > 0:   L(u) = 0.5 u^2 if |u| <= kappa else kappa (|u| - 0.5 kappa)
 *                rho_ij = |tau_i - [u_ij<0]| L(u_ij) / kappa
 *                dtheta_i = -(w_b / N) sum_j |tau_i - [u_ij<0]| clip(u_ij, -kappa, kappa) / kappa
 *   kappa == 0:  rho_ij = |tau_i - [u_ij<0]| |u_ij|          (plain quantile regression)
 *                dtheta_i = -(w_b / N) sum_j (tau_i - [u_ij<0])
 *   loss_b = (1 / N) sum_i sum_j rho_ij;  loss_rows[b] = w_b loss_b (the rows sum to the loss);
 *   priorities[b] = clip(loss_b, 1e-6, 1e6), unweighted.
 * dtheta has pred's shape: the rows of the other actions and the padding columns are written as exact zeros; dueling:
 * the gradient w.r.t. the advantage rows and the value row (through the merge).  The target net gets no gradient.
 * Summation order: for each i, four partial sums over j = w, w + 4, ... (w = 0 .. 3, ascending j, from 0), combined as
 * ((p0 + p1) + p2) + p3; the loss then sums over i as the butterfly above.  Deterministic: no atomics.
 * actions_b >= n_actions is read as n_actions - 1.  kappa < 0 or not finite: ARL_E_ARG.                            */
int arl_qrdqn_loss(const float* pred, const float* tgt_next, const float* pol_next_or_null, const uint8_t* actions,
                   const float* returns, const uint8_t* terminals, const float* is_weights_or_null, int64_t batch,
                   int32_t n_actions, int32_t n_quantiles, int32_t q_stride, int32_t dueling, float gamma_n, float kappa,
                   float* dtheta, float* loss_rows, float* priorities, void* stream);

/* ------------------------------------------------------------------------- *
 * Implicit quantile networks (IQN)
 * ------------------------------------------------------------------------- */

/* IQN (Dabney et al. 2018, "Implicit Quantile Networks for Distributional RL"; the reference has none): the quantile
 * fractions tau ~ U(0, 1) are drawn per sample, embedded with cosine features and multiplied into the conv features;
 * the network's output holds one row per (sample, fraction) and one column per action:
 *   theta f32[batch][R][a_stride], a_stride % 4 == 0, a_stride >= n_actions; the padding columns are ignored.
 * The five entry points below refuse with ARL_E_ARG (-1), before any HIP call and with no output written: a NULL
 * mandatory pointer, a size below 1, more than ARL_IQN_MAX_FRACTIONS (64) fractions per sample, more than 64 actions,
 * a_stride % 4 != 0, a_stride < n_actions or > 2^20, batch or rows x R (row0 included) above 2^31 - 1, f % 4 != 0,
 * f > 2^24, batch x R x f > 2^40, kappa negative or not finite, and arl_iqn_embed given neither or both of tau_in / state.  A vector operand
 * (psi, phi, x, g, dphi, dpsi, cosf) not 16-byte aligned: ARL_E_ALIGN.  Plain fp32, no atomics, deterministic.   */
#define ARL_IQN_COS 64                      /* cosine features per fraction (the paper's n = 64)               */
#define ARL_IQN_MAX_FRACTIONS 64
#define ARL_IQN_PHILOX_STREAM 0xC9514E31u   /* second key word; csrc/noisy.hip's streams are all below 2^31    */
/* Philox streams by second key word: 2 layer + which (< 2^31): csrc/noisy.hip's layer noise; ARL_IQN_PHILOX_STREAM:
 * the fractions below; ARL_AUG_PHILOX_STREAM (0xA5D3F1C7): arl_replay_extract_shift's shift offsets.              */

/* Fractions and their cosine features for rows x R (sample, fraction) pairs, pair (row, r) at p = row R + r:
 *   tau f32[rows R], cosf f32[rows R][64], cosf[p][i] = cos(pi i tau[p]), i = 0 .. 63 (Eq. 4 of the paper, i = 0 included)
 * given mode (tau_in != NULL, state == NULL): tau[p] = tau_in[p].
 * drawn mode (state = int64[2] (seed, counter) != NULL, tau_in == NULL; the kernel only READS state):
 *   e = (row0 + row) R + r; call = state[1] + call_offset (two's complement int64)
 *   words = Philox4x32-10(key = ((uint32) seed, ARL_IQN_PHILOX_STREAM),
 *                         counter = ((uint32)(e / 4), 0, (uint32) call, (uint32)(call >> 32)))
 *   k = words[e % 4] >> 9 (23 bits);  tau = (2 k + 1) * 2^-24: exact in fp32, never 0 or 1.
 *   row0 / call_offset let a chunked pass and the passes of one update read disjoint parts of the streams.
 * Cosine: the argument is reduced in integers.  |tau| = s 2^e (s its 24-bit significand): the angle i tau (in units of
 * pi) is i s 2^e exactly; it is taken modulo 2 and folded by cos(2 - t) = cos t, cos(1 - t) = -cos t and
 * cos(1/2 - t) = sin t to t in [0, 1/4], all on integers, then cospif(t) or sinpif(t) of the device library is taken.
 * t is a multiple of tau's last place 2^e and at most 1/4, so it has at most 24 significant bits (converts exactly)
 * whenever |tau| >= 2^-3 or tau is a drawn fraction (last place 2^-24); below that -- 25 bits in [2^-4, 2^-3), 26 in
 * [2^-5, 2^-4), one more per binade -- it is rounded once to fp32 (relative 2^-24).  |tau| < 2^-14 is not folded at
 * all (i tau < 2^-8).  The sign of tau_in is ignored (cos is even) and a subnormal tau_in is reduced like any other
 * value.  i = 0 gives exactly 1, an odd multiple of 1/2 exactly 0.  A tau_in of magnitude 2^24 or more is an even
 * integer (cos = 1); a tau_in that is not finite is not checked and also gives 1. */
int arl_iqn_embed(const float* tau_in_or_null, const int64_t* state_or_null, int64_t row0, int64_t call_offset,
                  int64_t rows, int32_t r, float* tau, float* cosf, void* stream);

/* The merge x[b R + r][f] = psi[b][f] * phi[b R + r][f] (psi f32[batch][f] the rectified conv features, phi
 * f32[batch R][f] the rectified embedding) and its backward pass for g = d loss / d x, f32[batch R][f]:
 *   dphi[b R + r][f] = g[b R + r][f] * psi[b][f] where phi[b R + r][f] > 0, else 0
 *   dpsi[b][f] = sum_r g[b R + r][f] * phi[b R + r][f] where psi[b][f] > 0, else 0; r ascending, the sum starts at 0.
 * Both are the pre-activation gradients of the layers below.  One lane per float4 along f, the r loop inside it.   */
int arl_iqn_merge_fwd(const float* psi, const float* phi, int64_t batch, int32_t r, int32_t f, float* x, void* stream);
int arl_iqn_merge_bwd(const float* g, const float* psi, const float* phi, int64_t batch, int32_t r, int32_t f,
                      float* dphi, float* dpsi, void* stream);

/* Action serving: Q_a = (sum_k theta(k, a)) / K in fp32, k ascending, the sum starts at 0; greedy action = FIRST maximum
 * (a = 0, then every a whose Q_a > the best so far); override, the one-hot row and `greedy` exactly as arl_qrdqn_act.
 * state_or_null != NULL: after its own work one thread does state[1] += advance (the last launch of a pass that drew
 * fractions; no launch of that pass reads state afterwards).
 *   theta f32[batch][K][a_stride]; onehot f32[batch][n_actions]; greedy u8[batch] or NULL                            */
int arl_iqn_act(const float* theta, const int32_t* override_or_null, int64_t batch, int32_t n_actions, int32_t k,
                int32_t a_stride, float* onehot, uint8_t* greedy_or_null, int64_t* state_or_null, int64_t advance,
                void* stream);

/* Pairwise quantile-Huber loss at drawn fractions, with its gradient.  pred f32[batch][N][a_stride] at fractions
 * tau_pred f32[batch][N]; tgt_next, pol_next_or_null f32[batch][N'][a_stride].  Per sample b,
 * w_b = (is_weight_b or 1) / batch, keep = 1 - terminal_b, L the Huber function of arl_qrdqn_loss:
 *   a*     = first maximum over a of Q_a (as arl_iqn_act, K = N') under pol_next if given (double DQN), else tgt_next
 *   T_j    = returns_b + keep * (gamma_n * theta_tgt(j, a*))                      (fp32, in this order)
 *   u_ij   = T_j - theta_pred(i, actions_b);  [u<0] = 1 for u < 0, else 0 (u == 0 counts as not negative)
 *   kappa > 0:   rho_ij = |tau_i - [u_ij<0]| L(u_ij) / kappa
 *                dtheta_i = -(w_b / N') sum_j |tau_i - [u_ij<0]| clip(u_ij, -kappa, kappa) / kappa
 *   kappa == 0:  rho_ij = |tau_i - [u_ij<0]| |u_ij|
 *                dtheta_i = -(w_b / N') sum_j (tau_i - [u_ij<0])
 *   loss_b = (1 / N') sum_i sum_j rho_ij;  loss_rows[b] = w_b loss_b;  priorities[b] = clip(loss_b, 1e-6, 1e6).
 * dtheta f32[batch][N][a_stride]: column actions_b of row i holds dtheta_i, everything else exact zeros.
 * Summation order: for each i, four partial sums over j = w, w + 4, ... (w = 0 .. 3, ascending j, each from 0),
 * combined as ((p0 + p1) + p2) + p3: no chain is longer than N' / 4 + 3 additions.  The loss then sums over i as a
 * butterfly over the 64 lanes (lane ^ 32, ^ 16, ... ^ 1; lanes >= N add 0).  One 256-thread workgroup per sample.
 * actions_b >= n_actions is read as n_actions - 1.  state_or_null / advance as in arl_iqn_act.                      */
int arl_iqn_loss(const float* pred, const float* tau_pred, const float* tgt_next, const float* pol_next_or_null,
                 const uint8_t* actions, const float* returns, const uint8_t* terminals,
                 const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n, int32_t n_target,
                 int32_t a_stride, float gamma_n, float kappa, float* dtheta, float* loss_rows, float* priorities,
                 int64_t* state_or_null, int64_t advance, void* stream);

/* Munchausen IQN (Vieillard, Pietquin, Geist 2020, "Munchausen Reinforcement Learning"): arl_iqn_loss with a soft-max
 * bootstrap and the scaled, clipped log-policy bonus added to the reward.  tgt_next, tgt_cur f32[batch][N'][a_stride]:
 * the TARGET net on next_obs and on obs.  tau_e > 0 the entropy temperature, alpha >= 0 the bonus scale, l0 <= 0 the
 * clip floor (the paper: 0.03, 0.9, -1).  For a row Q[0 .. A) of action values, in fp32 with expf / logf of the device
 * library:
 *   v = max_a Q_a;  c_a = Q_a - v;  e_a = expf(c_a / tau_e);  s = sum_a e_a
 *   lp_a = c_a - tau_e * logf(s)      (= tau_e log pi_a: finite even where pi_a underflows to 0);   pi_a = e_a / s
 * Per sample b:
 *   Q^next_a = (sum_j tgt_next(j, a)) / N', j ascending, the sum starts at 0 (as arl_iqn_act); Q^cur likewise of tgt_cur
 *   m_b    = alpha * clip(lp^cur_{actions_b}, l0, 0)                               (on terminal rows too)
 *   soft_j = sum_a pi^next_a * (tgt_next(j, a) - lp^next_a)                        a ascending, the sum starts at 0
 *   T_j    = (returns_b + m_b) + keep * (gamma_n * soft_j)                         (in this order)
 * and from T_j on everything is arl_iqn_loss: u_ij, rho_ij, dtheta, loss_rows, priorities, their summation orders, the
 * actions_b >= n_actions rule, state_or_null / advance.  No action is selected by an argmax; there is no double-DQN form.
 * Summation order of the soft-max: lane = action; v and s are butterflies over the 64 lanes (lane ^ 32, ^ 16, ... ^ 1;
 * lanes >= A add 0 to s and take no part in the maximum).  One 256-thread workgroup per sample; the [N'][A] tile of
 * tgt_next is staged in LDS.  With alpha == 0 and a maximum of Q^next unique by a gap of at least 88 tau_e (so that every
 * other e_a is 0): s == 1, soft_j == tgt_next(j, a*), and the outputs equal arl_iqn_loss's (pol_next NULL) bit for bit.
 * Refusals as arl_iqn_loss's, and ARL_E_ARG for tau_e not finite or <= 0, alpha not finite or < 0, l0 not finite or > 0. */
int arl_miqn_loss(const float* pred, const float* tau_pred, const float* tgt_next, const float* tgt_cur,
                  const uint8_t* actions, const float* returns, const uint8_t* terminals,
                  const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n, int32_t n_target,
                  int32_t a_stride, float gamma_n, float kappa, float tau_e, float alpha, float l0, float* dtheta,
                  float* loss_rows, float* priorities, int64_t* state_or_null, int64_t advance, void* stream);

/* ------------------------------------------------------------------------- *
 * Fully parameterized quantile functions (FQF)
 * ------------------------------------------------------------------------- */

/* FQF (Yang et al. 2019, "Fully Parameterized Quantile Function for Distributional RL"; the reference has none): the
 * implicit quantile network above, with the fractions neither fixed nor drawn but proposed per state by one dense layer
 * on the conv features (N logits per sample) and trained to minimise the 1-Wasserstein distance to the network's own
 * quantile function (the paper's Algorithm 1: ONE set of fractions per sample, used for every pass of that sample).
 *   logits, dlogits f32[batch][n_stride], n_stride % 4 == 0, n_stride >= N; the padding columns of logits are ignored
 *   theta f32[batch][N][a_stride] as above; tau f32[batch][N + 1]; tau_hat, q, logq f32[batch][N]; 1 <= N <= 64
 * The three entry points below refuse with ARL_E_ARG (-1), before any HIP call and with no output written: a NULL
 * mandatory pointer, a size below 1, more than ARL_IQN_MAX_FRACTIONS fractions, more than 64 actions, a_stride % 4 != 0,
 * a_stride < n_actions or > 2^20, n_stride % 4 != 0, n_stride < N or > 2^20, batch or batch x (N + 1) above 2^31 - 1,
 * kappa or ent_coef negative or not finite.  logits / dlogits -- the operands the dense kernels read and write as
 * vectors -- not 16-byte aligned: ARL_E_ALIGN.  Plain fp32 (expf / logf of the device library), no atomics, no
 * generator: deterministic.
 *
 * Fractions of one sample from its N logits l_k (one wave per sample, lane = k):
 *   v = max_k l_k;  c_k = l_k - v;  e_k = expf(c_k);  s = sum_k e_k
 *       (v and s: butterflies over the 64 lanes, lane ^ 32, ^ 16, ... ^ 1; lanes >= N add 0 and take no part in the maximum)
 *   q_k = e_k / s;  logq_k = c_k - logf(s)                       (finite where q_k underflows to 0)
 *   tau_0 = 0;  tau_{i+1} = min(tau_i + q_i, 1), i = 0 .. N - 2, SEQUENTIALLY with i ascending (every lane walks the
 *       same chain);  tau_N = 1 exactly
 *   tau_hat_i = 0.5 (tau_i + tau_{i+1}), i = 0 .. N - 1;  tau_mid = (tau_1 .. tau_{N-1}), compact f32[batch][N - 1]
 *   H = 0 - sum_k q_k logq_k                                     (the same butterfly)
 * so tau is non-decreasing, inside [0, 1], and tau_i <= tau_hat_i <= tau_{i+1}.  N == 1: q = 1, logq = 0, H = 0,
 * tau = (0, 1), tau_hat = 0.5, and tau_mid is not written.  tau and tau_hat are mandatory; tau_mid, q, logq, entropy
 * (what serving does not need) may be NULL.                                                                        */
int arl_fqf_fractions(const float* logits, int64_t batch, int32_t n, int32_t n_stride, float* tau, float* tau_hat,
                      float* tau_mid_or_null, float* q_or_null, float* logq_or_null, float* entropy_or_null,
                      void* stream);

/* Action serving: arl_iqn_act with the probability-weighted mean Q_a = sum_k (tau_{k+1} - tau_k) * theta(k, a) in fp32, k
 * ascending, the sum starts at 0 (a zero weight -- repeated fractions -- contributes an exact 0); first maximum,
 * override, the one-hot row and `greedy` exactly as arl_iqn_act.  Nothing is drawn: there is no state to advance.
 *   theta f32[batch][K][a_stride] (the net at tau_hat); tau f32[batch][K + 1]                                       */
int arl_fqf_act(const float* theta, const float* tau, const int32_t* override_or_null, int64_t batch,
                int32_t n_actions, int32_t k, int32_t a_stride, float* onehot, uint8_t* greedy_or_null, void* stream);

/* Quantile-Huber loss at the proposed fractions and the fraction loss's gradient, in one launch.  pred
 * f32[batch][N][a_stride]: the online net on obs at tau_hat; pred_mid f32[batch][N - 1][a_stride]: the online net on obs at
 * tau_1 .. tau_{N-1} (NULL allowed when N == 1: never read); tgt_next, pol_next_or_null f32[batch][N][a_stride]: the
 * target / online net on next_obs at the SAME tau_hat; tau, tau_hat, q, logq, entropy: arl_fqf_fractions' outputs.
 * Per sample b, w_b = (is_weight_b or 1) / batch, w_j = tau_{j+1} - tau_j:
 *   a*     = first maximum over a of sum_j w_j * sel(j, a), j ascending, the sum starts at 0 (as arl_fqf_act);
 *            sel = pol_next if given (double DQN), else tgt_next
 *   T_j    = returns_b + keep * (gamma_n * theta_tgt(j, a*))
 * and from T_j on everything is arl_iqn_loss with tau_pred = tau_hat and N' = N -- the same device function: u_ij,
 * rho_ij, dtheta, loss_rows, priorities, their summation orders, the kappa == 0 form, the actions_b >= n_actions rule.
 * With equal inputs and an equal a*, dtheta, loss_rows and priorities equal arl_iqn_loss's bit for bit.
 * Fraction loss (Proposition 1 of the paper; it sends no gradient into pred or pred_mid), with theta(.) the taken
 * action's column:
 *   g_i      = (2 * pred_mid(i) - pred(i)) - pred(i - 1),  i = 1 .. N - 1                (= d W1 / d tau_i)
 *   G        = sum_{i=1}^{N-1} g_i * tau_i,  i ascending, the sum starts at 0
 *   S_k      = sum_{i=k+1}^{N-1} g_i,  i ascending, the sum starts at 0                  (S_{N-1} = 0)
 *   dlogits_k = w_b * (q_k * (S_k - G) + ent_coef * (q_k * (logq_k + H))),  k = 0 .. N - 1   (minimises W1 - ent_coef H)
 *   frac_rows[b] = w_b * G
 * frac_rows is a surrogate whose gradient w.r.t. the logits is the fraction loss's; its VALUE is not W1.  Columns
 * N .. n_stride - 1 of dlogits are written as exact zeros; N == 1 gives all-zero dlogits and frac_rows = 0.  One 256-thread
 * workgroup per sample: waves 0, 1, 3 as arl_iqn_loss, wave 2 (lane = k) takes the fraction part.                  */
int arl_fqf_loss(const float* pred, const float* pred_mid_or_null, const float* tau, const float* tau_hat,
                 const float* q, const float* logq, const float* entropy, const float* tgt_next,
                 const float* pol_next_or_null, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                 const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n, int32_t a_stride,
                 int32_t n_stride, float gamma_n, float kappa, float ent_coef, float* dtheta, float* loss_rows,
                 float* priorities, float* dlogits, float* frac_rows, void* stream);

/* Plain DQN action serving: greedy action = first maximum of the Q row (T.argmax), override as
 * above, one-hot row out.  Replaces AtariDqnPolicy.get_actions / actions_sym,
 * accel_rl/policies/dqn/atari_dqn_policy.py:61-63,76-79,118-130.
 *   q f32[batch][q_stride], q_stride % 4 == 0 >= n_actions (<= 255); onehot f32[batch][n_actions]
 * dueling != 0 (dqn_cnn.py:89-112): columns 0..n_actions-1 are advantages, column n_actions the
 *   value; q_a = val + (adv_a - mean adv).                                                  */
int arl_dqn_act(const float* q, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                int32_t q_stride, int32_t dueling, float* onehot, uint8_t* greedy_or_null, void* stream);

/* Loss of DQN.build_loss, accel_rl/algos/dqn/dqn.py:137-172: next_q = max_a target(next_obs) or
 * (double DQN) target(next_obs)[argmax_a policy(next_obs)]; y = return + (1 - terminal) gamma^n
 * next_q; d = y - q[action]; 0.5 d^2, or the Huber loss with threshold delta_clip (> 0);
 * importance-weighted mean; priorities = clip(|d|, 0, delta_clip) (|d| when delta_clip <= 0).
 *   out: dq f32[batch][q_stride] (d mean-loss / d q; zero outside the taken action),
 *        loss_rows f32[batch] (their sum is the loss), td_abs f32[batch]
 * dueling != 0: rows as in arl_dqn_act; dq is the gradient w.r.t. advantages and value.        */
int arl_dqn_loss(const float* q, const float* tgt_next_q, const float* pol_next_q_or_null,
                 const uint8_t* actions, const float* returns, const uint8_t* terminals,
                 const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t q_stride,
                 int32_t dueling, float gamma_n, float delta_clip, float* dq, float* loss_rows, float* td_abs,
                 void* stream);

/* DrQ (Kostrikov, Yarats, Fergus 2020; the reference has none): arl_dqn_loss with the target averaged over k shifted
 * views of next_obs and the loss over m shifted views of obs (arl_replay_extract_shift's view-major rows):
 *   q, dq f32[m * batch][q_stride]; tgt_next_q, pol_next_q_or_null f32[k * batch][q_stride];
 *   actions, returns, terminals, is_weights_or_null, loss_rows, td_abs [batch]
 * One lane per sample b, everything inside the lane and in this order:
 *   next_q_i = arl_dqn_loss's next_q of row i * batch + b (first maximum of the online row -- double DQN -- or of the
 *              target row, valued by the target row; dueling rows merged as in arl_dqn_act), i = 0 .. k - 1
 *   nbar     = next_q_0 if k == 1, else (((next_q_0 + next_q_1) + ...) + next_q_{k-1}) / (float) k
 *   y        = returns_b + keep * (gamma_n * nbar)
 *   for v = 0 .. m - 1:  d_v = y - q(v * batch + b)[actions_b];  loss_v, its slope and row v * batch + b of dq exactly
 *              as arl_dqn_loss computes them, under the weight w = ((is_weight_b or 1) / (float) batch) / (float) m
 *   loss_rows[b] = ((w loss_0 + w loss_1) + ...), starting from its first term
 *   td_abs[b]    = ((p_0 + p_1) + ...) / (float) m,  p_v = |d_v| clipped as arl_dqn_loss's td_abs
 * The device code of a row is arl_dqn_loss's own; with k == m == 1 all three outputs equal arl_dqn_loss's bit for bit.
 * Sizes and refusals as arl_dqn_loss, plus (ARL_E_RANGE) k or m outside 1 .. 8 and m * batch or k * batch >= 2^31.
 * A refused call launches nothing.                                                                                  */
int arl_drq_loss(const float* q, const float* tgt_next_q, const float* pol_next_q_or_null, const uint8_t* actions,
                 const float* returns, const uint8_t* terminals, const float* is_weights_or_null, int64_t batch,
                 int32_t m, int32_t k, int32_t n_actions, int32_t q_stride, int32_t dueling, float gamma_n,
                 float delta_clip, float* dq, float* loss_rows, float* td_abs, void* stream);

/* Munchausen DQN (Vieillard, Pietquin, Geist 2020): arl_dqn_loss with a soft-max bootstrap and the scaled, clipped
 * log-policy bonus added to the reward.  tgt_next_q, tgt_cur_q f32[batch][q_stride]: the TARGET net on next_obs and on
 * obs (dueling rows merged as in arl_dqn_act).  With v, c_a, e_a, s, lp_a, pi_a of a row as defined at arl_miqn_loss
 * (tau_e > 0, alpha >= 0, l0 <= 0; expf / logf of the device library, fp32):
 *   m_b    = alpha * clip(lp^cur_{actions_b}, l0, 0)                               (on terminal rows too)
 *   soft_b = sum_a pi^next_a * (q^next_a - lp^next_a)                              a ascending, the sum starts at 0
 *   y_b    = (returns_b + m_b) + keep * (gamma_n * soft_b)                         (in this order)
 *   d_b    = y_b - q(obs)[actions_b]
 * and from d_b on everything is arl_dqn_loss: squared or Huber loss, importance weights, dq (through the dueling merge),
 * loss_rows, td_abs.  No action is selected by an argmax; there is no double-DQN form.  One lane per sample: the
 * maximum, then s with a ascending from 0, then soft_b, all inside the lane.  With alpha == 0 and a maximum of q^next
 * unique by a gap of at least 88 tau_e: s == 1, soft_b == max_a q^next_a, and the outputs equal arl_dqn_loss's
 * (pol_next_q NULL) bit for bit.  Sizes as arl_dqn_loss (ARL_E_RANGE); a NULL mandatory pointer, tau_e not finite or
 * <= 0, alpha not finite or < 0, l0 not finite or > 0: ARL_E_ARG.  A refused call launches nothing.                  */
int arl_mdqn_loss(const float* q, const float* tgt_next_q, const float* tgt_cur_q, const uint8_t* actions,
                  const float* returns, const uint8_t* terminals, const float* is_weights_or_null, int64_t batch,
                  int32_t n_actions, int32_t q_stride, int32_t dueling, float gamma_n, float delta_clip, float tau_e,
                  float alpha, float l0, float* dq, float* loss_rows, float* td_abs, void* stream);

/* Regression of Q on given targets (PQN, Gallici et al. 2024, "Simplifying Deep Temporal Difference Learning"; the
 * reference has none): arl_dqn_loss's TD row against a target that is an input.  Row i of the minibatch:
 *   src = idx_or_null ? idx_or_null[i] : i;  a = actions[src] (read as n_actions - 1 if >= n_actions);  y = returns[src]
 *   d = y - q[i][a]
 * and from d on everything is arl_dqn_loss's (its device code, not a copy): 0.5 d^2 or the Huber loss with threshold
 * delta_clip (> 0), its slope, under the weight w = 1 / (float) batch; no dueling merge, no importance weights.
 *   q, dq f32[batch][q_stride]; actions u8[n], returns f32[n] with every src < n (the caller answers for idx)
 *   out: dq (zero outside column a), loss_rows f32[batch] (their sum is the loss), td_abs f32[batch] (|d|, clipped to
 *        delta_clip when that is > 0)
 * Sizes as arl_dqn_loss (1 <= n_actions <= 255, q_stride >= n_actions and % 4 == 0, 1 <= batch < 2^31; else
 * ARL_E_RANGE); a NULL mandatory pointer: ARL_E_ARG.  A refused call launches nothing.                              */
int arl_q_regress_loss(const float* q, const int32_t* idx_or_null, const uint8_t* actions, const float* returns,
                       int64_t batch, int32_t n_actions, int32_t q_stride, float delta_clip, float* dq,
                       float* loss_rows, float* td_abs, void* stream);

/* ------------------------------------------------------------------------- *
 * Soft actor-critic for discrete actions (SAC-Discrete)
 * ------------------------------------------------------------------------- */

/* SAC-Discrete (Christodoulou 2019, "Soft Actor-Critic for Discrete Action Settings"; the reference has none): an actor
 * that puts out one logit per action, two critics with a target copy each, and a learned temperature alpha =
 * expf(log_alpha).  csrc/sac.hip.  Every row is f32[batch][stride] as arl_dqn_loss's: stride % 4 == 0, stride >=
 * n_actions (<= 255); padding columns are ignored on input and written as exact zeros on output.  For a row z[0 .. A) of
 * logits, with v, c_a, e_a, s, lp_a, pi_a as defined at arl_miqn_loss and tau_e = 1 (the device code arl_mdqn_loss runs;
 * fp32, expf / logf of the device library):
 *   m = max_a z_a;  e_a = expf(z_a - m);  s = sum_a e_a, a ascending, the sum starts at 0
 *   lp_a = (z_a - m) - logf(s)   (finite where pi_a underflows to 0);   pi_a = e_a / s
 * One lane per sample in all three entry points; every sum over the actions is taken inside the lane, a ascending, from 0.
 *
 * Action serving.  prob f32[batch][n_actions] (compact, as arl_dqn_act's onehot):
 *   deterministic == 0:  prob[b][a] = pi_a -- the sampler's categorical kernel (arl_sample_categorical) draws from it
 *   deterministic != 0:  a one-hot row at the FIRST maximum of the logits
 *   override_or_null[b] >= 0 forces a one-hot row at that action in either mode
 *   greedy_or_null[b] = the first maximum in either mode
 * Sizes as arl_dqn_act without dueling, batch < 2^31 (ARL_E_RANGE); NULL logits or prob: ARL_E_ARG.                    */
int arl_sacd_act(const float* logits, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                 int32_t stride, int32_t deterministic, float* prob, uint8_t* greedy_or_null, void* stream);

/* The critics', the actor's and the entropy's rows of one minibatch, in ONE launch.  q1, q2: the online critics on obs;
 * q1t_next, q2t_next: the TARGET critics on next_obs; logits, logits_next: the actor on obs and on next_obs; log_alpha
 * f32[1] on the device, read inside the kernel (a captured graph sees every update of it).  Per sample b, with
 * alpha = expf(log_alpha[0]), w = (is_weight_b or 1) / (float) batch, keep = 1 - terminal_b, pi', lp' of logits_next and
 * pi, lp of logits:
 *   soft   = sum_a pi'_a * (fminf(q1t_next_a, q2t_next_a) - alpha * lp'_a)          a ascending, the sum starts at 0
 *   y      = returns_b + keep * (gamma_n * soft)                                    (in this order)
 *   d_i    = y - q_i[actions_b],  i = 1, 2
 *   the loss L(d_i) (0.5 d^2, or the Huber loss with threshold delta_clip > 0), its slope into dq_i[actions_b] and the
 *   clipped |d_i| = p_i exactly as arl_dqn_loss computes them (the same device function) under the weight w; every
 *   other column of dq_i: exact zero
 *   stats[0][b] = q_loss_rows = w * L(d_1) + w * L(d_2);   stats[1][b] = td_abs = (p_1 + p_2) / 2
 *   g_a    = alpha * lp_a - fminf(q1_a, q2_a);   J = sum_a pi_a * g_a                a ascending, the sum starts at 0
 *   dlogits[b][k] = (pi_k * (g_k - J)) / (float) batch,  k < n_actions;  exact zeros in the padding
 *   stats[2][b] = pi_loss_rows = J / (float) batch;   stats[3][b] = ent_rows = -(sum_a pi_a * lp_a)
 * stats is f32[4][batch], contiguous: its first two rows are the adjacent (loss rows | priorities) pair of arl_dqn_loss's
 * callers.  The actor's loss sends no gradient into the critics and is not importance-weighted.  actions_b >= n_actions
 * is read as n_actions - 1.  With log_alpha = -inf (alpha == 0), q2t_next == q1t_next and logits_next ahead at the
 * maximum of q1t_next by a gap of at least 88: soft == that maximum, and dq1 and td_abs equal arl_dqn_loss's on
 * (q1, q1t_next) (pol_next_q NULL) bit for bit.  No atomics: two launches on the same inputs give the same bits.
 * Sizes as arl_dqn_loss without dueling, batch < 2^31 (ARL_E_RANGE); a NULL mandatory pointer, gamma_n or delta_clip not
 * finite: ARL_E_ARG.  A refused call launches nothing and writes nothing.                                              */
int arl_sacd_loss(const float* q1, const float* q2, const float* q1t_next, const float* q2t_next, const float* logits,
                  const float* logits_next, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                  const float* is_weights_or_null, const float* log_alpha, int64_t batch, int32_t n_actions,
                  int32_t stride, float gamma_n, float delta_clip, float* dq1, float* dq2, float* dlogits, float* stats,
                  void* stream);

/* Gradient of the temperature loss alpha * (H - H_target) with respect to log_alpha, H the batch mean of arl_sacd_loss's
 * ent_rows (entropy above the target lowers alpha):
 *   grad_out[0] = expf(log_alpha[0]) * (S / (float) batch - target_entropy);   grad_out[1 .. 3] = 0
 * grad_out f32[4] (a 16-byte optimiser range with one entry in use).  Summation order of S, fixed and atomic-free: ONE
 * 256-thread workgroup; thread t adds ent_rows[t], ent_rows[t + 256], ... to 0 in ascending order; the 256 partial sums
 * p_t are then folded as p_t += p_{t + h} for t < h, h = 128, 64, ... 1, and S = p_0.  1 <= batch < 2^31 (ARL_E_RANGE);
 * a NULL pointer or a target_entropy that is not finite: ARL_E_ARG.  A refused call launches nothing.                  */
int arl_sacd_alpha_grad(const float* ent_rows, int64_t batch, const float* log_alpha, float target_entropy,
                        float* grad_out, void* stream);

/* Q(lambda) returns of an on-policy Q-learner (PQN), computed backwards over a rollout from the CURRENT network.  Rows
 * env-major as in arl_gae_scan: row e * horizon + t.
 *   q        f32[n_env * horizon][q_stride]   the network on the rollout's observations
 *   q_last   f32[n_env][q_stride]             the network on the observations after the last step
 *   rewards  f32[n_env * horizon]   dones u8[n_env * horizon] (0 / non-zero)   returns f32[n_env * horizon] (out)
 * m(row) = fp32 maximum of the row's first n_actions entries (fmaxf, exact; a NaN entry is skipped).
 * b_t = (double) m(q row (e, t + 1)) for t < T - 1, b_{T-1} = (double) m(q_last row e).  R is carried in float64, in
 * exactly this expression order and without contraction:
 *   t = T - 1:  R = (double) r_t + (done_t ? 0.0 : discount * b_t)
 *   t < T - 1:  R = (double) r_t + (done_t ? 0.0 : discount * (b_t + lambda * (R_next - b_t)))
 * and returns[e * T + t] = (float) R at every step: equal to a float64 restatement bit for bit.  One wave per env: the
 * row maxima in parallel, one lane walks the T steps.  Indexing is 64-bit.
 * Refused before any HIP call, nothing written: a NULL pointer (ARL_E_ARG); n_env outside 1 .. 2^31 - 1, horizon
 * outside 1 .. 4096, n_actions outside 1 .. 64, q_stride < n_actions, not a multiple of 4 or > 2^20 (ARL_E_RANGE);
 * discount or lambda not finite or outside [0, 1], returns overlapping an input (ARL_E_ARG); q or q_last not 16-byte,
 * rewards or returns not 4-byte aligned (ARL_E_ALIGN).                                                               */
int arl_qlambda_scan(const float* q, const float* q_last, const float* rewards, const uint8_t* dones, double discount,
                     double lambda, int64_t n_env, int32_t horizon, int32_t n_actions, int32_t q_stride,
                     float* returns, void* stream);

/* V-trace value targets and policy-gradient advantages (IMPALA, Espeholt et al. 2018), computed backwards over a
 * rollout from the CURRENT network against the behaviour policy the sampler recorded.  Rows env-major as in
 * arl_gae_scan: row e * horizon + t.
 *   prob         f32[n_env * horizon][n_actions]   the current policy on the rollout's observations (arl_pg_head_infer)
 *   old_prob     f32[n_env * horizon][n_actions]   the behaviour policy
 *   actions      u8[n_env * horizon]               a byte >= n_actions is read as n_actions - 1
 *   values       f32[n_env * horizon]              the current value head on the rollout's observations
 *   last_values  f32[n_env]                        ... on the observations after the last step
 *   rewards      f32[n_env * horizon]   dones u8[n_env * horizon] (0 / non-zero)
 *   returns      f32[n_env * horizon] (out)        the value targets vs
 *   advantages   f32[n_env * horizon] (out)        the policy-gradient advantages, importance weight included
 *   stats_or_null f32[n_env][2] (out, optional)    [0] = the sum of ratio over the env's steps, added in float64 in walk
 *                                                  order (t = T - 1 .. 0, from 0.0) and rounded once; [1] = the number of
 *                                                  steps with ratio > rho_bar
 * Everything is float64, in exactly this expression order and without contraction.  Per step, a = min(actions[row],
 * n_actions - 1), p = prob[row][a], m = old_prob[row][a]:
 *   ratio = ((double) p + 1e-8) / ((double) m + 1e-8)
 *   rho = ratio < rho_bar ? ratio : rho_bar;  cw = ratio < c_bar ? ratio : c_bar;  pg = ratio < pg_rho_bar ? ratio : pg_rho_bar
 *   g   = done_t ? 0.0 : discount
 * The walk runs t = T - 1 .. 0 per env; acc_next and vs_next are carried as doubles, never as the rounded floats that
 * were stored.  At t = T - 1: acc_next = 0.0, v_next = vs_next = (double) last_values[e]; below, v_next = (double) V_{t+1}.
 *   q_v   = (double) r_t + g * v_next
 *   delta = rho * (q_v - (double) V_t)
 *   acc   = delta + ((g * (lambda * cw)) * acc_next)
 *   vs    = (double) V_t + acc
 *   adv   = pg * (((double) r_t + g * vs_next) - (double) V_t)
 *   returns[row] = (float) vs;  advantages[row] = (float) adv
 * equal to a float64 restatement bit for bit (float64 division is correctly rounded).  Inputs are taken as finite
 * (probabilities >= 0): nothing is checked on the device.  One wave per env: ratios in parallel, one lane walks the T
 * steps; no atomics, two launches give the same bits.  Indexing is 64-bit.
 * Refused before any HIP call, nothing written: a NULL pointer other than stats_or_null (ARL_E_ARG); n_env outside
 * 1 .. 2^31 - 1, horizon outside 1 .. 4096, n_actions outside 1 .. ARL_MAX_ACTIONS (ARL_E_RANGE); discount or lambda not
 * finite or outside [0, 1], rho_bar, c_bar or pg_rho_bar not finite or <= 0, an output overlapping an input or another
 * output (ARL_E_ARG); a float pointer not 4-byte aligned (ARL_E_ALIGN).                                              */
int arl_vtrace_scan(const float* prob, const float* old_prob, const uint8_t* actions, const float* values,
                    const float* last_values, const float* rewards, const uint8_t* dones, double discount, double lambda,
                    double rho_bar, double c_bar, double pg_rho_bar, int64_t n_env, int32_t horizon, int32_t n_actions,
                    float* returns, float* advantages, float* stats_or_null, void* stream);

/* ------------------------------------------------------------------------- *
 * R2D2 (Kapturowski et al. 2019; the reference has none): replayed sequences from a stored recurrent state.
 * csrc/r2d2.hip.  A sequence is U = burn_in + train_len + n consecutive steps of one environment's ring
 * (arl_replay: `size` steps per environment); sequences start at the ring indices that are multiples of the sequence
 * stride S (slot k starts at step k * S; size % S == 0), and rows are laid out [sequence][time].
 * ------------------------------------------------------------------------- */

/* Append side, ONE launch, no arithmetic (states are copied bit for bit).  From one sampler batch (env-major: row
 * e * horizon + t; step t of the batch lands on ring index (idx + t) mod size, as arl_replay_append's idx):
 *   state_store[s][e][((idx + t) mod size) / S][:] = state_in[s][e * horizon + t][:]   for every t with
 *                                                    ((idx + t) mod size) % S == 0: the state BEFORE that step
 *   reset_ring[e][(idx + t) mod size]              = resets[e * horizon + t]           for every t
 *   state_in / state_store: HOST arrays of n_state (0 .. 2) device pointers, f32[n_env * horizon][hidden] and
 *   f32[n_env][size / S][hidden], 16-byte aligned (else ARL_E_ALIGN; both may be NULL with n_state == 0);
 *   resets u8[n_env * horizon]; reset_ring u8[n_env][size].
 * Null pointers: ARL_E_ARG.  ARL_E_RANGE, nothing launched and no output written: n_env, horizon, size or seq_stride
 * < 1, horizon % seq_stride != 0, size % seq_stride != 0, horizon > size, idx outside 0 .. size - 1, n_state outside
 * 0 .. 2, hidden % 4 != 0, hidden > 1024.  One workgroup per environment: a latency-bound launch.                   */
int arl_seq_store(const float* const* state_in, int32_t n_state, int32_t hidden, const uint8_t* resets,
                  int32_t n_env, int32_t horizon, int32_t size, int32_t seq_stride, int32_t idx,
                  float* const* state_store, uint8_t* reset_ring, void* stream);

/* Sample side, ONE launch, no arithmetic.  env i32[batch], slot i32[batch] (the sum tree's, or the host's, on the
 * device); for sequence j and t = 0 .. seq_len - 1:
 *   env_rows[j * seq_len + t]   = env[j]
 *   step_rows[j * seq_len + t]  = (slot[j] * S + t) mod size            the lists arl_replay_extract takes
 *   resets_out[j * seq_len + t] = reset_ring[env[j]][that step]
 *   state_out[s][j][:]          = state_store[s][env[j]][slot[j]][:]    the state BEFORE the sequence's first step
 *   state_store / state_out: HOST arrays of n_state (0 .. 2) device pointers, f32[n_env][size / S][hidden] and
 *   f32[batch][hidden], 16-byte aligned (else ARL_E_ALIGN).  (env, slot) pairs may repeat.
 * The CALLER guarantees 0 <= env[j] < n_env and 0 <= slot[j] < size / S: the numbers live on the device, the host
 * cannot check them and the kernel clamps nothing (and asserts nothing).
 * Null pointers: ARL_E_ARG.  ARL_E_RANGE, nothing launched and no output written: batch, seq_len, size or seq_stride
 * < 1, size % seq_stride != 0, batch * seq_len > 2^31 - 1, n_state outside 0 .. 2, hidden % 4 != 0, hidden > 1024.
 * One workgroup per sequence: a latency-bound launch.                                                                */
int arl_seq_prepare(const int32_t* env, const int32_t* slot, int32_t batch, int32_t seq_len, int32_t size,
                    int32_t seq_stride, const float* const* state_store, int32_t n_state, int32_t hidden,
                    const uint8_t* reset_ring, int32_t* env_rows, int32_t* step_rows, float* const* state_out,
                    uint8_t* resets_out, void* stream);

/* R2D2's loss, its gradient and the sequence priorities in ONE launch.  U = burn_in + train_len + n; row (b, t) is row
 * b * U + t.
 *   q, q_tgt     f32[batch * U][q_stride]   the online and the target network on the same rows; dueling != 0: rows as
 *                                           in arl_dqn_act (q_a = val + (adv_a - mean adv))
 *   actions      u8[batch * U]              a byte >= n_actions is read as n_actions - 1 (arl_dqn_loss indexes with
 *                                           the byte as it is; here no access leaves the row)
 *   returns      f32[batch * U]             the replay memory's n-step discounted return
 *   terminals    u8[batch * U]              terminal inside the n-step window, as arl_replay_extract reports it
 *   is_weights_or_null f32[batch]
 * Everything is float64 from the float32 inputs, in exactly this expression order and without contraction, rounded to
 * float32 once per output.  A merged entry is (double) val + ((double) adv_a - mean), mean = (0.0 + adv_0 + adv_1 ...)
 * / (double) n_actions.  For every sequence b and train step t = burn_in .. burn_in + train_len - 1:
 *   a*   = first maximum over a of q[b, t + n, a]                     (merged if dueling)
 *   x    = q_tgt[b, t + n, a*]                                        (merged if dueling)
 *   hinv = x                                                          if rescale_eps <= 0, else, with e = rescale_eps,
 *        = sign(x) * (dl * (dl + 2.0)),  dl = (2.0 * |x|) / ((s + 1.0) + 2.0 * e),
 *                                        s  = sqrt(1.0 + (4.0 * e) * ((|x| + 1.0) + e))
 *          (the closed form ((s - 1) / (2 e))^2 - 1 of h's inverse, written without its cancellation near x = 0:
 *          u = (s - 1) / (2 e) has u - 1 = dl, because s^2 = (1 + 2 e)^2 + 4 e |x|, and u^2 - 1 = dl (dl + 2))
 *   z    = returns[b, t] + (terminals[b, t] ? 0.0 : gamma_n * hinv)
 *   y    = z                                                          if rescale_eps <= 0, else
 *        = sign(z) * (sqrt(|z| + 1.0) - 1.0) + e * z                  (sign(0) = 0)
 *   d    = y - q[b, t, action]                                        (merged if dueling)
 * and with w_b = (is_weights[b] or 1.0) / (double) (batch * train_len), the sums and the maximum walked in time order
 * from 0.0:
 *   td_abs f32[batch][train_len] = |d|
 *   loss_rows f32[batch]         = w_b * sum_t 0.5 * (d * d)
 *   priorities f32[batch]        = eta * max_t |d| + (1.0 - eta) * ((sum_t |d|) / (double) train_len)
 *   dq f32[batch * U][q_stride]  = the gradient of sum_b loss_rows[b] w.r.t. q: g = -(w_b * d) in the taken action's
 *                                  column of a train row; dueling: through the merge, g - g / A in the taken
 *                                  advantage, -(g / A) in the others, g in the value column.  Exact +0 in every
 *                                  burn-in row, every one of the n trailing rows, every padding column and (without
 *                                  dueling) every other action.  The target carries no gradient.
 * loss_rows and priorities need not be adjacent, but may be.  One 64-lane wave per sequence: lanes take train steps
 * l, l + 64, ...; one lane walks the sums; no atomics, two launches give the same bits.  Indexing is 64-bit.
 * Refused before any HIP call, nothing written: a NULL pointer other than is_weights_or_null, gamma_n, rescale_eps
 * or eta not finite (ARL_E_ARG); batch < 1, train_len outside 1 .. 1024, burn_in outside 0 .. 1024, n outside
 * 1 .. ARL_REPLAY_MAX_HORIZON, n_actions outside 1 .. 255, q_stride % 4 != 0, q_stride < n_actions + (dueling != 0),
 * batch * U > 2^31 - 1 (ARL_E_RANGE); dq not 16-byte or another float pointer not 4-byte aligned (ARL_E_ALIGN).       */
int arl_r2d2_loss(const float* q, const float* q_tgt, const uint8_t* actions, const float* returns,
                  const uint8_t* terminals, const float* is_weights_or_null, int32_t batch, int32_t burn_in,
                  int32_t train_len, int32_t n, int32_t n_actions, int32_t q_stride, int32_t dueling, double gamma_n,
                  double rescale_eps, double eta, float* dq, float* td_abs, float* loss_rows, float* priorities,
                  void* stream);

/* ------------------------------------------------------------------------- *
 * LayerNorm + rectifier between the contraction launches (PQN's Q-network)
 * ------------------------------------------------------------------------- */

/* Row-wise over z f32[rows][width], contiguous (NHWC conv activation: rows = B * Ho * Wo, width = channels; dense
 * layer: rows = B, width = units); gamma, beta f32[width].  fp32, no contraction, per row in this order:
 *   mean = (sum_j z_j) / (float) width;  var = (sum_j (z_j - mean)^2) / (float) width  (two passes over the row in
 *   registers, biased);  rstd = 1 / sqrtf(var + eps);  xhat_j = (z_j - mean) * rstd;
 *   y_j = max(0, gamma_j * xhat_j + beta_j)
 * Lanes and summation order (fixed: two launches are bit-identical; DESIGN.md 22 derives the error bound from it).
 * A row is held by LPR consecutive lanes of one wave, V float4s per lane; lane l holds float4 number v * LPR + l:
 *   width 4 .. 32: LPR 8, V 1 | 36 .. 64: LPR 16, V 1 | 68 .. 256: LPR 64, V 1 | 260 .. 512: LPR 64, V 2 |
 *   516 .. 1024: LPR 64, V 4
 * A row sum: per lane s = q_0, then s = s + q_v (v ascending), q_v = ((x + y) + z) + w of float4 v (0 past the row's
 * end); then the butterfly s = s + s[lane ^ off], off = LPR / 2, LPR / 4, .. 1, after which every lane of the row holds
 * the same bits.  Every element passes through at most D = 4 V + log2(LPR) additions.
 * A block of 256 threads holds RPB = 256 / LPR row slots, slot k in its threads k * LPR .. k * LPR + LPR - 1 (a wave holds
 * 64 / LPR consecutive slots); a slot past the last row computes on zeros and stores nothing.  The forward takes
 * min(2048, ceil(rows / RPB)) blocks, slot k of block b walking the rows b * RPB + k + i * grid * RPB; no result of it
 * depends on that grid.
 * Forward: writes y (a second buffer: z is KEPT, y == z is refused -- the backward pass recomputes xhat from z and
 * stats, so nothing but stats, 8 bytes per row, is stored for it beyond the activations) and stats f32[rows][2] =
 * (mean, rstd).
 * Backward: g_j = dy_j [y_j > 0], h_j = g_j * gamma_j, xhat_j = (z_j - mean) * rstd with the forward's stats,
 *   m1 = (sum_j h_j) / (float) width, m2 = (sum_j h_j * xhat_j) / (float) width   (row sums as above)
 *   dz_j = rstd * ((h_j - m1) - xhat_j * m2)                        dz may be dy itself (in place) or another buffer
 *   dgamma_j = sum_rows g_j * xhat_j,  dbeta_j = sum_rows g_j
 * dy_masked = 1: dy already carries the mask (masked-out entries +0, as the data-gradient launches leave them): it is
 * taken as it comes and y is not read; the mask being idempotent, the outputs equal the dy_masked = 0 call's bit for bit.
 * The column sums: slot k of block b adds the terms of rows b * RPB + k + i * grid * RPB (one fp32 product g_j * xhat_j
 * per dgamma term), i ascending, to an accumulator that starts at +0, grid = min(256, ceil(rows / RPB)); the block adds
 * its RPB slots in slot order (slot 0's accumulator, then + slot 1's, ..; a slot without a row holds +0) into one
 * partial row, part f32[grid][width] for dgamma followed by the same for dbeta in `workspace`
 * (>= arl_ln_bwd_workspace_bytes()); arl_fold_many adds the partial rows in its fixed order -- at once (items2_or_null
 * NULL: a second launch here) or later (items2_or_null: two arl_fold_item are filled in, the workspace stays live until
 * the caller's arl_fold_many).  No atomics; bit-identical run to run.  Indexing is 64-bit.
 * Refused before any HIP call, nothing written: a NULL pointer (items2_or_null excepted), dy_masked not 0 / 1, eps not
 * finite or <= 0, y == z (ARL_E_ARG); rows outside 1 .. 2^31 - 1, width outside 4 .. 1024 or not a multiple of 4
 * (ARL_E_RANGE); any pointer not 16-byte aligned (ARL_E_ALIGN).                                                      */
int64_t arl_ln_bwd_workspace_bytes(void);
int arl_ln_relu_fwd(const float* z, const float* gamma, const float* beta, int64_t rows, int32_t width, float eps,
                    float* y, float* stats, void* stream);
int arl_ln_relu_bwd(const float* dy, const float* y, const float* z, const float* stats, const float* gamma,
                    int64_t rows, int32_t width, int32_t dy_masked, float* dz, float* dgamma, float* dbeta,
                    void* workspace, struct arl_fold_item* items2_or_null, void* stream);

/* ------------------------------------------------------------------------- *
 * Max pooling and the residual sum between the contraction launches (the IMPALA residual network)
 * ------------------------------------------------------------------------- */

/* 3 x 3 window, stride 2, padding 1 on every side (the padding never wins: it counts as -inf), on an NHWC activation
 * z f32[batch][in_h][in_w][channels]; out_h = (in_h - 1) / 2 + 1, out_w = (in_w - 1) / 2 + 1 (integer division).
 * Forward, per output element (b, oy, ox, c): best = -inf, arg = 0; for ky = 0, 1, 2 and, inside, kx = 0, 1, 2 with
 * iy = 2 oy - 1 + ky, ix = 2 ox - 1 + kx inside the image: v = z[b][iy][ix][c]; if (v > best) { best = v; arg = 3 ky + kx; }
 * -- the FIRST maximum in row-major window order keeps its place (strict >), which is torch.nn.functional.max_pool2d's
 * rule.  The window's centre always lies inside the image, so with finite inputs (they are taken as finite; nothing is
 * checked on the device) best is an element of z.
 *   y f32[batch][out_h][out_w][channels] = best
 *   y_relu_or_null (same shape)          = best > 0 ? best : +0     (the next convolution's input and rectifier mask)
 *   arg_or_null u8 (same shape)          = arg
 * Backward, a gather with one thread per four input elements: dz[b][i][j][c] = the sum of dy[b][oy][ox][c] over the
 * windows (oy, ox) with i / 2 <= oy <= min((i + 1) / 2, out_h - 1), j / 2 <= ox <= min((j + 1) / 2, out_w - 1) -- the at
 * most four that contain (i, j) -- whose arg equals 3 (i - 2 oy + 1) + (j - 2 ox + 1), taken with oy ascending and, inside,
 * ox ascending: the first such term as it is, every further one added to the sum so far; +0 where there is none.  Every
 * element of dz is written.
 * No atomics, no partial sums: two launches give the same bits.  Indexing is 64-bit.
 * Refused before any HIP call, nothing written: a NULL pointer other than the two optional ones, y, y_relu or z the same
 * buffer, dz == dy (ARL_E_ARG); batch outside 1 .. 2^20, in_h or in_w outside 1 .. 2^16, channels outside 4 .. 1024 or
 * not a multiple of 4 (ARL_E_RANGE); a float pointer not 16-byte aligned, arg not 4-byte aligned (ARL_E_ALIGN).      */
int arl_maxpool3s2_fwd(const float* z, int64_t batch, int32_t in_h, int32_t in_w, int32_t channels, float* y,
                       float* y_relu_or_null, uint8_t* arg_or_null, void* stream);
int arl_maxpool3s2_bwd(const float* dy, const uint8_t* arg, int64_t batch, int32_t in_h, int32_t in_w, int32_t channels,
                       float* dz, void* stream);

/* sum[i] = a[i] + b[i] (one fp32 addition) and, with relu_or_null, relu[i] = sum[i] > 0 ? sum[i] : +0, i < n.  sum may be
 * a or b (a thread reads its own elements before it writes them); relu is a buffer of its own.
 * Refused before any HIP call, nothing written: a, b or sum NULL, relu equal to a, b or sum (ARL_E_ARG); n outside
 * 4 .. 2^40 or not a multiple of 4 (ARL_E_RANGE); a pointer not 16-byte aligned (ARL_E_ALIGN).                       */
int arl_add_relu(const float* a, const float* b, int64_t n, float* sum, float* relu_or_null, void* stream);

/* arl_gather_scale_obs_nhwc for the observations it refuses: out f32[batch][plane_bytes][cp], cp = channels rounded up
 * to a multiple of 4, out[b][p][c] = (float) obs[r][c][p] * scale (one fp32 multiplication) with r = idx_or_null ?
 * idx_or_null[b] : b, and +0 for c >= channels; obs u8[.][channels][plane_bytes], any plane size (a byte per load: the
 * path of image sizes no Atari frame has).  Row numbers are taken as valid.
 * Refused before any HIP call, nothing written: obs or out NULL (ARL_E_ARG); batch outside 1 .. 2^24, channels outside
 * 1 .. 1024, plane_bytes outside 1 .. 2^24 (ARL_E_RANGE); idx not 4-byte or out not 16-byte aligned (ARL_E_ALIGN).    */
int arl_gather_scale_obs_nhwc_any(const uint8_t* obs, const int32_t* idx_or_null, int64_t batch, int32_t channels,
                                  int32_t plane_bytes, float scale, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * LSTM cell of the recurrent policies
 * ------------------------------------------------------------------------- */

/* Limits of the six cell entry points below (arl_{lstm,gru,rnn}_cell_{fwd,bwd}), checked on the host before any launch;
 * a refused call launches nothing and writes no output:
 *   - a mandatory pointer NULL: ARL_E_ARG;
 *   - 1 <= batch <= ARL_CELL_MAX_BATCH (2^24) and 1 <= hidden <= ARL_CELL_MAX_HIDDEN (2^20), else ARL_E_RANGE.  The
 *     kernels index a row with int (at most 4 hidden - 1 < 2^22) and rows / elements with int64_t
 *     (batch * hidden <= 2^44, batch * stride <= 2^52): no index of an accepted call overflows;
 *   - every *_stride is the element distance between consecutive rows of its array.  With batch > 1 the stride of
 *     every non-NULL strided array must be at least the row it addresses (4 hidden, 3 hidden or hidden, named per
 *     argument below) and at most ARL_CELL_MAX_STRIDE (2^28), else ARL_E_RANGE: rows may be padded, never overlap.
 *     With batch == 1 no stride is used and none is checked (a one-row tensor's row stride is arbitrary); the stride
 *     of a NULL optional array is ignored.
 *   - arrays without a stride argument are contiguous ([batch][row width]).
 * Every thread reads and writes only its own element (b, j) of every array, so an output may be the same buffer as an
 * input of the same shape and stride; the policies rely on dc_prev == dc_next (LSTM) and dh_prev == dh_dir (GRU).
 * Saturated gates give finite results: a sigmoid of exactly 0 or 1 and a tanh of exactly +-1 have zero gradient.   */
#define ARL_CELL_MAX_BATCH  ((int64_t)1 << 24)
#define ARL_CELL_MAX_HIDDEN (1 << 20)
#define ARL_CELL_MAX_STRIDE ((int64_t)1 << 28)

/* Elementwise part of FastLstmLayer.step, accel_rl/policies/layers.py:331-346: gate order
 * f, i, c~, o; f, i, o = sigmoid, c~ = tanh; c = f c_prev + i c~; h = o tanh(c).  gx = x W_x + b and
 * gh = h_prev W_h are the callers' dense products (gh may be NULL = zero; contiguous [batch][4 hidden]).  Every
 * *_stride is the element distance between consecutive rows, so a time slice of a [trajectory][time] batch can be
 * addressed in place.  gates (optional) receives the activated gates for the backward pass.
 * Rows: gx, gates 4 hidden; c_prev, h_out, c_out hidden.  Limits: see above. */
int arl_lstm_cell_fwd(const float* gx, int64_t gx_stride, const float* gh_or_null, const float* c_prev,
                      int64_t cprev_stride, int64_t batch, int32_t hidden, float* h_out, int64_t h_stride,
                      float* c_out, int64_t c_stride, float* gates_or_null, int64_t gates_stride, void* stream);

/* Backward of the above for one time step: dh (from the layers above, strided) + dh_rec (from step
 * t+1, contiguous) and dc_next (contiguous) -> pre-activation gate gradients dgates[B][4H] and dc_prev (contiguous).
 * Each of dh, dh_rec, dc_next may be NULL (= zero); with all three NULL dgates and dc_prev are all zero.  dc_prev may
 * be dc_next.  Rows: gates, dgates 4 hidden; dh, c_prev, c_out hidden.  Limits: see above. */
int arl_lstm_cell_bwd(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                      const float* dc_next_or_null, const float* gates, int64_t gates_stride,
                      const float* c_prev, int64_t cprev_stride, const float* c_out, int64_t c_stride,
                      int64_t batch, int32_t hidden, float* dgates, int64_t dgates_stride, float* dc_prev,
                      void* stream);

/* GRU cell (GruLayer.step, accel_rl/policies/layers.py:163-168), gate order r, u, c in the 3H-wide
 * arrays: r = s(gx_r + gh_r); u = s(gx_u + gh_u); c = tanh(gx_c + r gh_c); h = (1 - u) h_prev + u c.
 * gx = x [W_xr W_xu W_xc] + b, gh = h_prev [W_hr W_hu W_hc] (contiguous [batch][3 hidden]) are the callers' dense
 * products.  saved (optional, [B][4H]) receives r, u, c, gh_c for the backward pass.
 * Rows: gx 3 hidden; saved 4 hidden; h_prev, h_out hidden.  Limits: see above. */
int arl_gru_cell_fwd(const float* gx, int64_t gx_stride, const float* gh, const float* h_prev,
                     int64_t hprev_stride, int64_t batch, int32_t hidden, float* h_out, int64_t h_stride,
                     float* saved_or_null, int64_t saved_stride, void* stream);

/* Backward of one GRU step: dh (layers above, strided) + dh_rec + dh_dir (both contiguous, from
 * step t+1; each of the three may be NULL = zero) -> dgx[B][3H] (gradient wrt gx), dgh[B][3H] (wrt gh; its c block
 * carries the factor r) and dh_prev[B][H] (contiguous) = the direct part dh (1 - u); the caller adds dgh W_h^T.
 * dh_prev may be dh_dir.  The r column is dpc (gh_c (r (1 - r))): a saturated r gives 0 whatever gh_c is.
 * Rows: saved 4 hidden; dgx, dgh 3 hidden; dh, h_prev hidden.  Limits: see above. */
int arl_gru_cell_bwd(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                     const float* dh_dir_or_null, const float* saved, int64_t saved_stride,
                     const float* h_prev, int64_t hprev_stride, int64_t batch, int32_t hidden,
                     float* dgx, int64_t dgx_stride, float* dgh, int64_t dgh_stride, float* dh_prev,
                     void* stream);

/* Plain recurrent cell (RecurrentLayer.step, layers.py:80-82): h = tanh(gx + gh) (gh contiguous), and its backward
 * dpre = (dh + dh_rec) (1 - h^2) (dh strided, dh_rec contiguous, either may be NULL = zero).  Every row is hidden
 * wide.  Limits: see above. */
int arl_rnn_cell_fwd(const float* gx, int64_t gx_stride, const float* gh, int64_t batch, int32_t hidden,
                     float* h_out, int64_t h_stride, void* stream);
int arl_rnn_cell_bwd(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                     const float* h_out, int64_t h_stride, int64_t batch, int32_t hidden, float* dpre,
                     int64_t dpre_stride, void* stream);

/* ------------------------------------------------------------------------- *
 * Reset-aware BPTT: training a recurrent policy on a batch inside which environments were reset
 * ------------------------------------------------------------------------- */

/* Flag addressing shared by the four entry points below.  reset is u8[rows of the full batch], non-zero where the
 * recurrent state was set to zero AFTER that row's step.  Row b of a launch is compact row
 * flag_row0 + b * flag_row_step of a [trajectory][time] (mini)batch (flag_row0 = the time step, flag_row_step = the
 * horizon); its flag is reset[idx ? idx[compact row] : compact row], idx being arl_traj_minibatch's row map (or NULL:
 * the whole batch).  0 <= flag_row0, 1 <= flag_row_step and flag_row0 + (batch - 1) flag_row_step <= 2^31 - 1, else
 * ARL_E_RANGE; the caller answers for reset / idx covering those rows.
 *
 * arl_seq_handover: one launch hands the state of step t-1 (flag rows: those of step t-1) to step t of the learner's
 * forward scan.  Where the flag is set the previous state is +0, else the stored value bit for bit; no arithmetic.
 *   h_prev [B][H] strided -> hp [B][H] contiguous (the operand of h_prev W_h) and hprev_out [B][H] strided (the
 *   slice of step t of the array that feeds dW_h; also the GRU's elementwise h_prev);
 *   c_prev [B][H] strided -> cprev_out [B][H] strided (the LSTM's c_prev of step t, read by the cell and its
 *   backward); both NULL for cells with one state.
 * One float4 per lane: hidden % 4 == 0 and hidden <= 1024 (ARL_E_RANGE), every pointer 16-byte aligned and every
 * stride a multiple of 4 (ARL_E_ALIGN); batch and stride limits as for the cell entry points above.  A refused call
 * launches nothing.  Latency-bound (B x H elements); no throughput figure is claimed. */
int arl_seq_handover(const float* h_prev, int64_t h_stride, const float* c_prev_or_null, int64_t c_stride,
                     const uint8_t* reset, const int32_t* idx_or_null, int64_t flag_row0, int64_t flag_row_step,
                     int64_t batch, int32_t hidden, float* hp, float* hprev_out, int64_t hprev_stride,
                     float* cprev_out_or_null, int64_t cprev_out_stride, void* stream);

/* The three backward cells with the reset flags of THIS step's rows: where a row's flag is set, the gradients that
 * arrive from step t+1 (dh_rec; the LSTM's dc_next; the GRU's dh_dir) are left out for that row -- the arithmetic of
 * the plain entry point with those pointers NULL -- and everything else is the plain entry point's arithmetic in the
 * same order (one templated body).  c_prev / h_prev are the masked values arl_seq_handover wrote.  With
 * reset_or_null == NULL the plain entry point's own kernel is launched: the same bits.  Arguments, limits and
 * aliasing rules as for arl_{lstm,gru,rnn}_cell_bwd. */
int arl_lstm_cell_bwd_reset(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                            const float* dc_next_or_null, const float* gates, int64_t gates_stride,
                            const float* c_prev, int64_t cprev_stride, const float* c_out, int64_t c_stride,
                            int64_t batch, int32_t hidden, float* dgates, int64_t dgates_stride, float* dc_prev,
                            const uint8_t* reset_or_null, const int32_t* idx_or_null, int64_t flag_row0,
                            int64_t flag_row_step, void* stream);
int arl_gru_cell_bwd_reset(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                           const float* dh_dir_or_null, const float* saved, int64_t saved_stride,
                           const float* h_prev, int64_t hprev_stride, int64_t batch, int32_t hidden,
                           float* dgx, int64_t dgx_stride, float* dgh, int64_t dgh_stride, float* dh_prev,
                           const uint8_t* reset_or_null, const int32_t* idx_or_null, int64_t flag_row0,
                           int64_t flag_row_step, void* stream);
int arl_rnn_cell_bwd_reset(const float* dh_or_null, int64_t dh_stride, const float* dh_rec_or_null,
                           const float* h_out, int64_t h_stride, int64_t batch, int32_t hidden, float* dpre,
                           int64_t dpre_stride, const uint8_t* reset_or_null, const int32_t* idx_or_null,
                           int64_t flag_row0, int64_t flag_row_step, void* stream);

/* Optimiser state for ONE flat fp32 parameter bucket (all trainable params in
 * get_params order, accel_rl/optimizers/util.py:35-39). */
typedef struct arl_opt_state {
    int64_t n_params;
    float*  params;         /* f32[P] flat parameter vector (updated in place)   */
    float*  grads;          /* f32[P] flat gradient (after all-reduce in sync mode) */
    float*  slot0;          /* adam m / rmsprop accu                             */
    float*  slot1;          /* adam v / unused                                   */
    float*  step_count;     /* f32[1] Lasagne's t (floatX)                       */
    float*  lr_mult;        /* f32[1] device scalar (linear schedule, aac_base.py:165-168) */
    double* partials;       /* f64[ARL_OPT_PARTIALS] scratch                     */
    float*  grad_norm_log;  /* f32[norm_log_len] ring: norm of update k at k % len */
    int32_t norm_log_len;
} arl_opt_state;

#define ARL_OPT_PARTIALS 1024
#define ARL_OPT_ADAM     0
#define ARL_OPT_RMSPROP  1

/* grads *= avg_factor; norm = ||grads||_2; if clip > 0: grads *= clip(norm,0,clip)/(1e-7+norm);
 * then adam / rmsprop.  Two launches (sum of squares, fused update).
 * Replaces avg_grads_from_flat + apply_grad_norm_clip + lasagne update,
 * accel_rl/optimizers/util.py:63-76, sync/sync_ppo_optimizer.py:27-34; update
 * arithmetic as in accel_rl/optimizers/update_methods_stats.py:11-33 (rmsprop)
 * and :55-87 (adam).  clip <= 0, -0.0 and NaN mean "no clip" (norm still logged).
 *
 * The arithmetic, all float32, every operation rounded (the file is built without contraction; tests/optim_ref.py
 * restates it and tests/test_optim_limits_gpu.py holds the device to it bit for bit):
 *   lr = learning_rate * lr_mult[0];   norm = avg_factor * (float) sqrt(S), S the float64 sum of grads^2 (fixed order);
 *   cscale = fminf(fmaxf(norm, 0), clip) / (1e-7f + norm) if clip > 0 (not 1 below the clip: Lasagne's), else 1;
 *   gg = (g * avg_factor) * cscale;
 *   adam:    m = b1 m + (1 - b1) gg;  v = b2 v + (1 - b2) (gg gg);  p -= (a_t m) / (sqrtf(v) + eps),
 *            a_t = (lr sqrtf(1 - powf(b2, t))) / (1 - powf(b1, t));
 *   rmsprop: acc = rho acc + (1 - rho) (gg gg);  p -= (lr gg) / sqrtf(acc + eps).
 * A gradient that is not finite gives NaN where IEEE arithmetic gives NaN (with a clip: everywhere, through cscale).
 *
 * Limits, checked before anything is launched by EVERY entry point below that takes these arguments
 * (arl_corun_job_init included):
 *   ARL_E_ARG    a NULL state; NULL params, grads, slot0, step_count or lr_mult (arl_opt_step: or partials); a method
 *                other than ARL_OPT_ADAM / ARL_OPT_RMSPROP; adam without slot1; n_params <= 0; a log with
 *                norm_log_len <= 0;
 *   ARL_E_ALIGN  params, grads, slot0 or slot1 not 16-byte aligned (a range inside a larger bucket starts at a multiple
 *                of 4 elements);
 *   ARL_E_RANGE  adam: beta1 or beta2 outside [0, 1) (1 - beta^t would be 0); rmsprop: rho outside [0, 1]; epsilon or
 *                learning_rate negative or NaN.
 *
 * Lasagne's t is the float32 step_count[0]: the sum-of-squares launch adds 1 and the update reads it.  At 2^24 it stops
 * advancing (2^24 + 1 is not a float32): every later step sees t = 2^24.  The powers have underflowed to 0 long before
 * for any beta < 1 - 1e-5, so a_t == lr there and the update is unaffected; only the ring index stops moving.
 * Ring index of this entry point: the norm of the step that makes t goes to grad_norm_log[((int) t - 1) % norm_log_len].
 * grad_norm_log may be NULL (nothing else changes).                                                                  */
int arl_opt_step(const arl_opt_state* opt, int32_t method, float learning_rate,
                 float avg_factor, float clip, float beta1_or_rho, float beta2,
                 float epsilon, void* stream);

/* The same update WITHOUT norm clipping (PPO's default, accel_rl/algos/pg/ppo.py:24: grad_norm_clip=None) as ONE
 * launch: the sum of squares for the logged norm is taken in the update's own pass over the gradient.  A call of
 * the optimizer (`optimize`, accel_rl/optimizers/single/ppo_optimizer.py:58-75) issues updates k = 0 .. n-1 and
 * then arl_opt_finish(n), which writes grad_norm_log[k % norm_log_len] for all of them and settles step_count.
 *   step_pp    f32[2] zero-initialised (Lasagne's t, ping-pong between consecutive updates)
 *   norm_parts f64[ARL_OPT_NORM_SLOTS][ARL_OPT_NORM_BLOCKS] scratch; update k uses row k only, and every word of the
 *              row that arl_opt_finish reads is written by the update (it need not be cleared between calls)
 * Arithmetic and refusals as arl_opt_step with cscale = 1; t = step_pp[k & 1] + 1 (stuck at 2^24 likewise), written
 * to step_pp[(k + 1) & 1] and step_count.  Also refused: NULL step_pp or norm_parts (ARL_E_ARG); k outside
 * 0 .. ARL_OPT_NORM_SLOTS - 1 (ARL_E_RANGE) -- norm_parts must hold all ARL_OPT_NORM_SLOTS rows, the library cannot
 * see its size.
 * arl_opt_finish: n_updates outside 1 .. ARL_OPT_NORM_SLOTS: ARL_E_RANGE.  Ring index of this path: update k of the
 * call logs at grad_norm_log[k % norm_log_len] -- by its position in the call, not by t -- each from a workgroup of
 * its own, so with a log n_updates > norm_log_len is refused (ARL_E_RANGE: two updates would write one word in an
 * undefined order); without a log any n_updates in range is fine.  It reads step_pp[n_updates & 1] into both words
 * and step_count, and may be repeated.                                                                              */
#define ARL_OPT_NORM_SLOTS  64
#define ARL_OPT_NORM_BLOCKS 2048
int arl_opt_step_noclip(const arl_opt_state* opt, int32_t method, float learning_rate, float avg_factor,
                        float beta1_or_rho, float beta2, float epsilon, int32_t k, float* step_pp,
                        double* norm_parts, void* stream);
int arl_opt_finish(const arl_opt_state* opt, int32_t n_updates, float avg_factor, float* step_pp,
                   const double* norm_parts, void* stream);

/* The no-clip update in two parts, so that the bulk of it can leave the step's critical path: once the gradient of a
 * range [hole_first, hole_first + hole_count) of the bucket is final (spec 1: the first dense layer's 3.5 M weights,
 * written by its weight-gradient kernel long before the conv layers' backward ends), that range's update -- HBM-bound
 * streaming -- can run INSIDE the launch of a later MFMA-bound data-gradient kernel, in extra workgroups
 * (arl_corun_job below; inside the PPO step: the host launch 42.6 -> ~48 us, the step's own update launch
 * 19.9 -> 4.9 us), and the step ends with the update of the small rest.  part 0 = everything but the hole (advances t; hole_count = 0: the
 * plain arl_opt_step_noclip), part 1 = the hole as a launch of its own.  hole_first, hole_count multiples of 4.
 * Per element the arithmetic is arl_opt_step_noclip's; a call that used a hole ends with arl_opt_finish_split.
 * The hole may start at 0, end at the bucket's last float4 or be the whole bucket (part 0 then still updates the last
 * n_params % 4 elements and advances t).  Refused with ARL_E_ARG besides arl_opt_step_noclip's refusals: hole_first or
 * hole_count negative or no multiple of 4, a hole past the end of the bucket, part 1 with an empty hole;
 * arl_opt_finish_split: hole_count negative, above n_params or no multiple of 4.                                     */
int arl_opt_step_noclip_split(const arl_opt_state* opt, int32_t method, float learning_rate, float avg_factor,
                              float beta1_or_rho, float beta2, float epsilon, int32_t k, float* step_pp,
                              double* norm_parts, int64_t hole_first, int64_t hole_count, int32_t part, void* stream);
int arl_opt_finish_split(const arl_opt_state* opt, int32_t n_updates, float avg_factor, float* step_pp,
                         const double* norm_parts, int64_t hole_count, void* stream);
/* Part 1 of update k as a job that a data-gradient launch carries: arl_corun_job_init describes it (same arguments
 * as part 1 above; nothing is launched), arl_conv2d_bwd_data / arl_conv2d_bwd_pair take it as an argument -- the
 * launch's grid gets one extra workgroup per CU (the first of the grid; ARL_CORUN_BLOCKS overrides the count, a tuning
 * aid) that streams the update while the others keep the matrix pipe busy -- and report whether they ran it;
 * arl_corun_job_run runs it as its own launch (what the caller does when no launch took it), before part 0.
 * The job is plain data owned by the caller: nothing is pending inside the library, an abandoned job costs nothing.
 * arl_corun_job_init refuses what part 1 of arl_opt_step_noclip_split refuses (and a NULL job: ARL_E_ARG);
 * arl_corun_job_run(NULL): ARL_E_ARG.  A hosting launch that runs the part with fewer workgroups than it has norm
 * slots zero-fills the others.                                                                                       */
typedef struct arl_corun_job { int64_t opaque[40]; } arl_corun_job;
int arl_corun_job_init(arl_corun_job* job, const arl_opt_state* opt, int32_t method, float learning_rate,
                       float avg_factor, float beta1_or_rho, float beta2, float epsilon, int32_t k, float* step_pp,
                       double* norm_parts, int64_t hole_first, int64_t hole_count);
int arl_corun_job_run(const arl_corun_job* job, void* stream);

/* ------------------------------------------------------------------------- *
 * Noisy dense layers (NoisyNets, factorized Gaussian noise; csrc/noisy.hip)
 * ------------------------------------------------------------------------- */

/* NoisyDenseLayer.get_output_for with factorized=True, accel_rl/policies/dqn/layers/noisy_layer.py:100-147 (the noise
 * draws of :83-88 / :125-139, f of :10-11), for AtariNoisyNetDqnPolicy (policies/dqn/atari_noisy_net_dqn_policy.py:20-148):
 *   y = x W + b + f(e_out) * ((x * f(e_in)) W_sigma + b_sigma),   f(e) = sgn(e) sqrt(|e|)
 * which equals x (W + W_sigma * f(e_in) f(e_out)^T) + b + b_sigma * f(e_out) without a per-row weight matrix.
 *
 * Generator.  Element j of the e_in (which = 0) or e_out (which = 1) draw of noisy layer `layer` for the row group
 * g = row / rows_per_draw (rows_per_draw = 1: every row draws its own noise, common_noise=False; = rows of a call:
 * one draw per call, common_noise=True) at call counter n, with seed s:
 *   words w[0..3] = Philox4x32-10(counter = (j / 4, g, n mod 2^32, n >> 32), key = (s mod 2^32, 2 layer + which))
 *     (Random123's Philox4x32 with 10 rounds: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 *      0xBB67AE85; per round (hi0, lo0) = M0 c0, (hi1, lo1) = M1 c2, c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0),
 *      the key incremented before rounds 2..10)
 *   for the pair p = (j % 4) / 2: u1 = ((w[2p] >> 8) + 0.5) / 2^24, u2 = ((w[2p+1] >> 8) + 0.5) / 2^24 (in (0, 1)),
 *   r = sqrt(-2 ln u1) in double, e = r cos(2 pi u2) for even j, r sin(2 pi u2) for odd j, rounded to float once.
 * Factorized noise (noisy_layer.py:83-88,125-139): e_in has fan_in elements, e_out `units`.
 *   e_or_null / f_or_null f32[rows][width] (e, f(e)), words_or_null u32[rows][width] (the word element j used,
 *   w[j % 4]); at least one of them.                                                                                */
int arl_noisy_normals(int64_t seed, int64_t counter, int32_t layer, int32_t which, int64_t rows, int32_t width,
                      int32_t rows_per_draw, float* e_or_null, float* f_or_null, uint32_t* words_or_null,
                      void* stream);

/* One noisy layer of a forward pass for arl_noisy_noise. */
typedef struct arl_noisy_layer {
    float* fein;                /* f32[rows][fan_in]: f(e_in) of each row                                           */
    float* feout;               /* f32[rows][out_stride]: f(e_out) of each row; columns units .. out_stride-1 = 0    */
    const float* x;             /* f32[rows][fan_in]: the layer's input if it exists already, else NULL             */
    float* xs;                  /* f32[rows][fan_in]: x * f(e_in) (written when x is given)                         */
    int32_t fan_in;             /* multiple of 4                                                                    */
    int32_t units;              /* width of e_out                                                                   */
    int32_t out_stride;         /* stored columns of the layer's output: multiple of 4, >= units                    */
    int32_t layer;              /* the generator's layer index: 0 <= layer < 2^30 (the stream id is 2 layer + which)  */
} arl_noisy_layer;
#define ARL_NOISY_MAX_LAYERS 8

/* The noise of every noisy layer of one forward pass of `rows` rows in ONE launch: the draws of the generator above at
 * seed state[0] and call counter state[1] (int64[2] in device memory -- the policy's noise state; a replayed hipGraph
 * reads the current value), f(e_in), f(e_out) and x * f(e_in) where x is given.  This launch does not advance the
 * counter: a later launch of the same pass does (arl_noisy_dense_combine's state_or_null), so eager and captured runs
 * draw the same sequence.  Replaces the rng.normal draws of noisy_layer.py:83-88,125-139.
 * Refused as by arl_noisy_normals and arl_noisy_draws, nothing launched: a layer index < 0 or >= 2^30 (ARL_E_ARG);
 * rows x fan_in or rows x out_stride above 2^40 (ARL_E_RANGE).                                                      */
int arl_noisy_noise(const int64_t* state, const arl_noisy_layer* layers, int32_t n_layers, int64_t rows,
                    int32_t rows_per_draw, void* stream);

/* The layer's output from its two products as arl_conv2d_fwd's items have them (relu 0; W product with bias b, W_sigma
 * product with bias b_sigma: splits == 0 means finished, bias applied; splits > 0: folded here in arl_fold_many's order,
 * then the bias): y = relu?(P_w + f(e_out) * P_sigma), f32[rows][units] (noisy_layer.py:120-147, a hidden layer's
 * rectifier: noisy_net_dqn_cnn.py:64-76).  fein_next / xs_next (both or neither): xs_next = y * fein_next, the next
 * noisy layer's input times its f(e_in).  state_or_null: state[1] += 1 (the pass's last launch advances the counter).  */
int arl_noisy_dense_combine(const arl_fold_item* w_prod, const float* bias_or_null, const arl_fold_item* sigma_prod,
                            const float* b_sigma_or_null, const float* feout, int64_t rows, int32_t units, int32_t relu,
                            float* y, const float* fein_next_or_null, float* xs_next_or_null, int64_t* state_or_null,
                            void* stream);

/* Backward of the noise terms, given g = dL/dy f32[rows][units] with the layer's rectifier mask applied (T.grad of
 * noisy_layer.py:141-147): g2 = g * f(e_out); db[u] = sum_rows g, db_sigma[u] = sum_rows g2, rows summed in order
 * (no atomics).  dW = g^T x and dW_sigma = g2^T (x * f(e_in)) are arl_conv2d_bwd_pair's.                           */
int arl_noisy_dense_bwd_prep(const float* g, const float* feout, int64_t rows, int32_t units, float* g2, float* db,
                             float* db_sigma, void* stream);

/* dx = dx_w + f(e_in) * dx_sigma, f32[rows][fan_in]: the data gradient of a noisy layer from its two data products
 * (g W and g2 W_sigma, both already multiplied by the rectifier mask of the layer below by arl_conv2d_bwd_pair).
 * dx may alias dx_w.  fan_in % 4 == 0, 16-byte aligned pointers.                                                   */
int arl_noisy_dense_bwd_dx(const float* dx_w, const float* dx_sigma, const float* fein, int64_t rows, int32_t fan_in,
                           float* dx, void* stream);

/* ---- AtariNoisyNetCatDqnPolicy: CatDqnCnn (accel_rl/policies/dqn/networks/catdqn_cnn.py:40-99) with every DenseLayer a
 * factorized NoisyDenseLayer (noisy_layer.py:15-147).  Its noise, with the generator above (seed s, call counter n of
 * the pass, rows_per_draw as above), H = hidden units, A = actions, N = atoms, S = atom_stride, x_c = the conv output in
 * the internal (h, w, c) order:
 *   not dueling, hidden layers j = 0 .. J-1 and the output layer "action_atoms" = layer J:
 *     hidden j   e_in  = (layer j, which 0, elements 0 .. fan_in-1)  e_out = (layer j, which 1, elements 0 .. units-1)
 *     output     e_in  = (layer J, which 0, elements 0 .. H_last-1)  e_out of reference unit a N + i (action a, atom i)
 *                                                                    = (layer J, which 1, element a S + i) of a draw of
 *                                                                      A S elements (the stored, atom-padded layout)
 *   dueling (one hidden layer; layers numbered in CatDqnCnn's construction order hidden_0, action_atoms, hidden_Val_0,
 *   Val):
 *     hidden_0     e_in = (layer 0, which 0, 0 .. F-1)   e_out = (layer 0, which 1, 0 .. H-1)
 *     action_atoms e_in = (layer 1, which 0, 0 .. H-1)   e_out of unit a N + i = (layer 1, which 1, element a S + i)
 *     hidden_Val_0 e_in = (layer 2, which 0, 0 .. F-1)   e_out = (layer 2, which 1, 0 .. H-1)
 *     Val          e_in = (layer 3, which 0, 0 .. H-1)   e_out of atom i = (layer 3, which 1, element i) of S elements
 *   (F = fan_in of the first hidden layer, element k of a conv-output draw = x_c element k).  Every e_in / e_out of
 *   the network is its own (layer, which) stream.  One pass = one call counter; the pass's last combine (or, with the
 *   fused loss below, its last hidden layer's combine) advances it by one.                                        */

/* One (layer, which) draw of arl_noisy_draws: row r gets f(e_j) of elements j = 0 .. width-1 at f[r pitch + j]; with x
 * (which 0 only) also xs[r pitch + j] = x[r pitch + j] f(e_j).  width, pitch multiples of 4, pointers 16-byte aligned. */
typedef struct arl_noisy_draw {
    float* f;
    const float* x;             /* or NULL                                                                          */
    float* xs;                  /* written when x is given                                                          */
    int32_t width;
    int32_t pitch;              /* floats between rows of f, x and xs (>= width)                                   */
    int32_t layer;              /* the generator's layer index                                                      */
    int32_t which;              /* 0: e_in, 1: e_out                                                                */
} arl_noisy_draw;
#define ARL_NOISY_MAX_DRAWS 16

/* The noise of one forward pass as a list of draws in ONE launch (arl_noisy_noise's generalisation: a draw may fill a
 * column range of a wider buffer -- the two streams' halves of a dueling network's stacked layers).  Reads seed
 * state[0] and call counter state[1]; does not advance it.  Replaces the rng.normal draws of noisy_layer.py:83-88,
 * 125-139 for every noisy layer of catdqn_cnn.py:58-99.                                                            */
int arl_noisy_draws(const int64_t* state, const arl_noisy_draw* draws, int32_t n_draws, int64_t rows,
                    int32_t rows_per_draw, void* stream);

/* The stacked 2H hidden layer of the dueling network (units 0 .. split-1: hidden_0, split .. units-1: hidden_Val_0,
 * catdqn_cnn.py:58-66,77-86 as NoisyDenseLayers): y = relu?(P_w + f(e_out) * P_sigma) with P_w the one x W product
 * over all units (bias b) and P_sigma, per stream, its own (x f(e_in_stream)) W_sigma_stream product (b_sigma):
 * sigma_lo total rows x split, sigma_hi rows x (units - split).  Every item folded in arl_fold_many's order, then its
 * bias, as arl_noisy_dense_combine; fein_next / xs_next and state_or_null as there.                                */
int arl_noisy_duel_combine(const arl_fold_item* w_prod, const float* bias_or_null, const arl_fold_item* sigma_lo,
                           const arl_fold_item* sigma_hi, const float* b_sigma_or_null, const float* feout, int64_t rows,
                           int32_t units, int32_t split, int32_t relu, float* y, const float* fein_next_or_null,
                           float* xs_next_or_null, int64_t* state_or_null, void* stream);

/* arl_noisy_dense_bwd_prep for that layer: g2 = g * f(e_out) written as two contiguous blocks, g2_lo f32[rows][split]
 * and g2_hi f32[rows][units - split] (the per-stream sigma products' dy); db, db_sigma f32[units] (rows in order). */
int arl_noisy_duel_bwd_prep(const float* g, const float* feout, int64_t rows, int32_t units, int32_t split,
                            float* g2_lo, float* g2_hi, float* db, float* db_sigma, void* stream);

/* dx = (dx_w + f(e_in_lo) * dx_sigma_lo) + f(e_in_hi) * dx_sigma_hi, f32[rows][fan_in]: that layer's data gradient
 * (g W, g2_lo W_sigma_lo, g2_hi W_sigma_hi, each already masked by the rectifier below).  dx may alias dx_w.
 * fan_in % 4 == 0, 16-byte aligned pointers.                                                                       */
int arl_noisy_duel_bwd_dx(const float* dx_w, const float* dx_sigma_lo, const float* fein_lo, const float* dx_sigma_hi,
                          const float* fein_hi, int64_t rows, int32_t fan_in, float* dx, void* stream);

/* A noisy output layer's logits as the items of its two arl_conv2d_fwd products have them, from the source's first row on
 * (row = (n_actions + dueling) atom_stride floats): logit = [x W + b] + f(e_out) ([x f(e_in) W_sigma] + b_sigma). */
typedef struct arl_noisy_logit_src {
    const float* w_part;        /* x W: f32[w_splits][..] partial sums, or (w_splits == 0) finished values (bias in) */
    const float* bias_or_null;  /* b, added after the fold (w_splits > 0)                                           */
    const float* s_part;        /* (x f(e_in)) W_sigma, likewise                                                    */
    const float* b_sigma_or_null;
    const float* feout;         /* f32[rows][row]: f(e_out)                                                         */
    int64_t w_split_stride;     /* floats between splits (the fold item's total)                                    */
    int64_t s_split_stride;
    int32_t w_splits;           /* 0 .. ARL_NOISY_CATDQN_MAX_SPLITS                                                 */
    int32_t s_splits;
} arl_noisy_logit_src;
#define ARL_NOISY_CATDQN_MAX_SPLITS 128

/* The fused loss launch's limits: splits per product, actions, atoms.  A caller past them runs the unfused pair
 * (arl_noisy_dense_combine per pass, then arl_catdqn_loss), which takes any split count.                          */
int arl_noisy_catdqn_loss_limits(int32_t* max_splits, int32_t* max_actions, int32_t* max_atoms);

/* arl_catdqn_loss_parts for a noisy output layer (AtariNoisyNetCatDqnPolicy; cat_dqn.py:40-109 on the logits of
 * catdqn_cnn.py:67-99 with NoisyDenseLayers): every logit is folded and noised exactly as arl_noisy_dense_combine
 * (relu 0) computes it, operation for operation, then the dueling merge, softmax, double-DQN selection, projection,
 * loss, KL and dlogits as arl_catdqn_loss -- the same bits as that pair, in one launch instead of three.  It does
 * not touch the noise state: a caller that uses it advances each pass's counter in the pass's last hidden combine.
 * wt_items_or_null / n_wt as arl_catdqn_loss_parts.  ARL_E_RANGE past arl_noisy_catdqn_loss_limits.                 */
int arl_noisy_catdqn_loss_parts(const arl_noisy_logit_src* pred, const arl_noisy_logit_src* tgt_next,
                                const arl_noisy_logit_src* pol_next_or_null, const float* z, const uint8_t* actions,
                                const float* returns, const uint8_t* terminals, const float* is_weights_or_null,
                                int64_t batch, int32_t n_actions, int32_t n_atoms, int32_t atom_stride, int32_t dueling,
                                float v_min, float v_max, float gamma_n, float* dlogits, float* loss_rows, float* kl,
                                const struct arl_dgrad_wt* wt_items_or_null, int32_t n_wt, void* stream);

/* ------------------------------------------------------------------------- *
 * ACER (Wang et al. 2017, "Sample Efficient Actor-Critic with Experience Replay"; the reference has none).
 * csrc/acer.hip.  One network puts out a row f32[2S], S a multiple of 4 with S >= A (the policy uses S = A rounded up to
 * a multiple of 32): columns [0, A) are the logits z, columns [S, S + A) the action values Q; padding is ignored on
 * input and written as exact zeros on output.  pi_a and lp_a of a logit row are the fp32 soft-max and log-soft-max
 * defined at arl_sacd_loss (the same device function).  eps = 1e-6 (a double) wherever a probability is a divisor, as
 * in the public implementation.  All four entry points: plain C++ HIP, no atomics (two launches on the same
 * inputs give the same bits), 64-bit indexing, no host synchronisation; a refused call launches nothing and writes
 * nothing.
 * ------------------------------------------------------------------------- */

/* Retrace(lambda) targets of Q, computed backwards over a rollout from the CURRENT network against the behaviour policy
 * the sampler recorded.  Rows env-major: row e * horizon + t.
 *   prob       f32[n_env * horizon][A]   the current policy's soft-max rows (arl_sacd_act on the network output at
 *                                        stride 2S: the scan itself calls no device-library function)
 *   prob_last  f32[n_env][A]             ... on the observations after the last step
 *   q, q_last  the Q half of the network output on the same rows: entry (row, a) at q[row * q_stride + a]
 *   old_prob   f32[n_env * horizon][A]   the behaviour policy mu
 *   actions    u8[n_env * horizon]       a byte >= A is read as A - 1
 *   rewards    f32[n_env * horizon]      dones u8[n_env * horizon] (0 / non-zero)
 *   qret_out   f32[n_env * horizon] (out);  v_out_or_null f32[n_env * horizon] (out, optional)
 *   stats_or_null f32[n_env][2] (out, optional): [0] = the sum of rho over the env's steps, added in float64 in walk
 *              order (t = T - 1 .. 0, from 0.0) and rounded once; [1] = the number of steps with rho > 1
 * Everything is float64 from the promoted inputs on, in exactly this expression order and without contraction:
 *   V(row) = sum_a (double) prob[row][a] * (double) q[row][a]          a ascending, the sum starts at 0.0
 *   qret   = V(last row of env e), from prob_last and q_last
 *   for t = T - 1 .. 0, a = min(actions[row], A - 1):
 *     qret = (double) r_t + (done_t ? 0.0 : discount * qret)
 *     qret_out[row] = (float) qret;   v_out[row] = (float) V_t
 *     rho  = (double) prob[row][a] / ((double) old_prob[row][a] + eps)
 *     cbar = lambda * (rho < 1.0 ? rho : 1.0)
 *     qret = cbar * (qret - (double) q[row][a]) + V_t
 * qret is carried as a double across steps, never as the rounded float that was stored: equal to a float64 restatement
 * bit for bit.  One wave per env: V, rho and Q(a) of the steps in parallel, one lane walks the T steps.
 * Refused before any HIP call: a NULL pointer other than the two optional ones (ARL_E_ARG); n_env outside 1 .. 2^31 - 1,
 * horizon outside 1 .. 4096, n_actions outside 1 .. ARL_MAX_ACTIONS, q_stride < n_actions, not a multiple of 4 or > 2^20
 * (ARL_E_RANGE); discount or lambda not finite or outside [0, 1], an output overlapping an input or another output
 * (ARL_E_ARG); a float pointer not 4-byte aligned (ARL_E_ALIGN).                                                      */
int arl_acer_retrace_scan(const float* prob, const float* prob_last, const float* q, const float* q_last,
                          int32_t q_stride, const float* old_prob, const uint8_t* actions, const float* rewards,
                          const uint8_t* dones, double discount, double lambda, int64_t n_env, int32_t horizon,
                          int32_t n_actions, float* qret_out, float* v_out_or_null, float* stats_or_null, void* stream);

/* The output stage of one ACER minibatch in one launch, one lane per sample.
 *   out      f32[batch][2S]   the live network's output;   out_avg f32[batch][2S] the average network's on the same rows
 *                             (only its logits are read);  S = half_stride
 *   old_prob f32[n][A], actions u8[n], qret f32[n]: read at row src = idx_or_null ? idx_or_null[b] : b (the caller
 *                             answers for idx, as for arl_q_regress_loss)
 *   dout     f32[batch][2S] (out);   stats f32[5][batch] (out)
 * Per sample, with (fp32) pi, lp of out's logits and pibar of out_avg's, everything below in float64 from the promoted
 * values P_a = (double) pi_a, L_a = (double) lp_a, B_a = (double) pibar_a, Q_a, mu_a = (double) old_prob[src][a],
 * R = (double) qret[src], t = min(actions[src], A - 1); every sum over the actions runs a ascending and starts at 0.0:
 *   V     = sum_a P_a * Q_a;   adv = R - V
 *   rho_a = P_a / (mu_a + eps);   f = (rho_t < c ? rho_t : c) * adv
 *   w_a   = 1.0 - c / (rho_a + eps), replaced by 0.0 unless > 0.0
 *   g_a   = ((a == t ? f / (P_a + eps) : 0.0) + w_a * (Q_a - V)) - ent_coeff * (L_a + 1.0)
 *           (the gradient with respect to the probabilities of the truncated term, the bias-correction term and the
 *            entropy bonus; Q, V and the weights are constants)
 *   k_a   = -(B_a / (P_a + eps))
 *   kg    = sum_a k_a * g_a;   kk = sum_a k_a * k_a
 *   s     = kk > 0.0 ? max((kg - delta) / kk, 0.0) : 0.0      (kk == 0.0 -- an all-zero pibar row -- projects nothing)
 *   zs_a  = g_a - s * k_a;   pz = sum_a P_a * zs_a
 *   dout[b][j]     = (float) (-(P_j * (zs_j - pz)) / (double) batch),  j < A
 *   dout[b][S + t] = (float) ((q_coeff * (Q_t - R)) / (double) batch);  every other column: exact zero
 *   stats[0][b] = (float) (-(obj + ent_coeff * H) / batch), the policy-objective row, a diagnostic:
 *                 obj = f * L_t, then for a ascending obj = obj + ((w_a * (Q_a - V)) * P_a) * L_a;  H = -(sum_a P_a * L_a)
 *   stats[1][b] = (float) (((0.5 * q_coeff) * ((Q_t - R) * (Q_t - R))) / batch)
 *   stats[2][b] = (float) H;   stats[3][b] = (float) s;   stats[4][b] = (float) rho_t
 * Stated limits: delta = +inf switches the projection off (s == 0.0 exactly); c = +inf switches the correction term off
 * (w_a == 0.0) and leaves the importance weight untruncated.
 * Refused before any HIP call: a NULL pointer other than idx_or_null, c not > 0, delta not >= 0 (a NaN fails both), q_coeff
 * or ent_coeff not finite, dout or stats overlapping out, out_avg or one another (ARL_E_ARG); batch outside 1 .. 2^31 - 1,
 * n_actions outside 1 .. ARL_MAX_ACTIONS, half_stride < n_actions, not a multiple of 4 or > 2^19 (ARL_E_RANGE); a float
 * pointer or idx not 4-byte aligned (ARL_E_ALIGN).                                                                    */
int arl_acer_loss(const float* out, const float* out_avg, const float* old_prob, const uint8_t* actions,
                  const float* qret, const int32_t* idx_or_null, int64_t batch, int32_t n_actions, int32_t half_stride,
                  double c, double delta, double q_coeff, double ent_coeff, float* dout, float* stats, void* stream);

/* The average network's step over a flat bucket, fp32:
 *   beta = 1.0f - alpha (once, on the host);   avg[i] = (alpha * avg[i]) + (beta * params[i])
 * two rounded products and one rounded sum, never an fma.  16-byte accesses with a scalar tail where both pointers are
 * 16-byte aligned, 4-byte accesses otherwise: the same bits either way.
 * Refused: a NULL pointer, alpha outside [0, 1] or NaN, avg overlapping params (ARL_E_ARG); n outside 1 .. 2^31 - 1
 * (ARL_E_RANGE); a pointer not 4-byte aligned (ARL_E_ALIGN).                                                          */
int arl_acer_avg_step(float* avg, const float* params, int64_t n, float alpha, void* stream);

/* dst segment i = src segment index[i], i < n_seg; segments are seg_bytes long and contiguous, src holds n_src_seg of
 * them.  index is i32[n_seg] ON THE DEVICE (a captured graph replays with new draws); nothing is read back by the host,
 * so an index < 0 is taken as 0 and one >= n_src_seg as n_src_seg - 1.  16-byte copies where seg_bytes is a multiple of
 * 16 and src and dst are 16-byte aligned, byte copies otherwise.
 * Refused: a NULL pointer, dst overlapping src or index (ARL_E_ARG); n_seg or n_src_seg outside 1 .. 2^31 - 1, seg_bytes
 * outside 1 .. 2^31 (ARL_E_RANGE); index not 4-byte aligned (ARL_E_ALIGN).                                            */
int arl_gather_segments(const void* src, const int32_t* index, int64_t n_seg, int64_t n_src_seg, int64_t seg_bytes,
                        void* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACCEL_RL_HIP_H */

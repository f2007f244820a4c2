/*
 * rdv.h — C ABI of the MI355X-native batched rendezvous environment (librdv_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of cfdeinza/reinforcement-learning-rendezvous:
 * RendezvousEnv.step()/reset() (reference rendezvous_env.py:160-270) and the helper methods the
 * evaluators call after every step (get_observation :294, get_errors :451, check_collision :388,
 * check_success :406, dist_from_koz :510).  The reference has no native plugin interface; its
 * boundary is the Gym-0.21 Env API (rendezvous_env.py:10,133-144,160,223) wrapped into an SB3 VecEnv
 * (main.py:33-34).  A Python host binds these entry points with ctypes and
 * exposes them as an SB3-compatible VecEnv of N environments.
 *
 * Conventions
 *   - every function returns 0 on success or a negative RdvError; the message of the last failure on
 *     the calling thread is returned by rdv_last_error().  Nothing throws across this ABI.
 *   - all `float*`/`double*`/`uint8_t*`/`int32_t*` data arguments are DEVICE pointers owned by the
 *     caller (e.g. torch tensors' data_ptr()) unless the name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is enqueued
 *     asynchronously on it; nothing here synchronises except rdv_get_stats/rdv_destroy.
 *   - a handle is not thread-safe; different handles (device shards) may be used from different threads.
 *   - rdv_step performs no allocation.
 *   - quaternions are scalar-first (reference utils/quaternions.py:2).
 *
 * Stream capture (HIP graphs; tests/test_gpu_graphs.py, tests/test_gpu_lstm_graphs.py)
 *   Every call that only enqueues work on `stream` may be recorded into a graph (hipStreamBeginCapture ... EndCapture, torch.cuda.graph) and
 *   replayed; the tests pin rdv_step (every variant, the evaluator build, groups, general bodies), rdv_step_many, rdv_rollout (the
 *   persistent kernel and the loop forms), rdv_get_state, rdv_snapshot, rdv_policy_act, rdv_policy_value, rdv_gae,
 *   rdv_rollout_advantages, and the setters rdv_set_params, rdv_set_group_params and rdv_set_rigid_body; and the recurrent calls
 *   rdv_lstm_act, rdv_lstm_value (committing and not), rdv_lstm_get_state, rdv_lstm_set_state, rdv_lstm_reset_state, rdv_rollout and
 *   rdv_rollout_advantages with a recurrent handle, each with a plain handle and with a set.  A replay computes bit for bit
 *   what the same calls compute eagerly.  Make the calls once eagerly before recording them (lazily created handles and module loading
 *   stay out of the capture), and record on one stream.
 *   A recurrent handle's state (h, c), its pending episode-start flags and its scratch rows live in the handle's DEVICE allocation, and
 *   every call reads and writes them there, on `stream`: a graph freezes none of them.  A replay therefore continues from whatever the
 *   call before it — a replay or an eager call on the replaying stream (rdv_lstm_act, rdv_lstm_value, rdv_lstm_set_state,
 *   rdv_lstm_reset_state) — left there; rdv_lstm_set_weights and rdv_lstm_set_member_weights, made eagerly between replays, rewrite the
 *   block inside the handle's allocation, so the graph stays valid and its later replays use the new weights.
 *   WHAT A GRAPH FREEZES.  The library decides on the host, at call time, what a launch will be; a graph keeps those decisions:
 *     - the kernel chosen (variant, storage, on_done, diag / eval outputs, general bodies, groups, the first step after rdv_set_state);
 *     - whether a prepare launch goes in front of rdv_step_many / rdv_rollout (it does when something since the last one — rdv_step, a
 *       parameter change — left the prepared next-episode states behind);
 *     - seed, the reset tape, noise_seed and noise_counter0, and every pointer.  A replayed rdv_rollout / rdv_policy_act therefore
 *       REPEATS the noise counter of the recording: every replay draws the same noise for the same (env, step).  Eager calls that are to
 *       reproduce a replay pass that same counter; a learner that wants fresh noise per replay records rollouts with different counters.
 *   Calls that therefore INVALIDATE graphs recorded earlier on the handle (record again after them): rdv_seed, rdv_set_reset_tape,
 *   rdv_set_kernel_variant, rdv_set_state / rdv_restore, rdv_set_param_groups, and rdv_set_rigid_body when it switches the handle
 *   between general and non-general bodies.
 *   Calls that REFUSE inside a capture (RDV_ERR_INVALID_ARGUMENT, the message says "stream capture"; asked before anything touches the
 *   stream, so the capture stays valid): rdv_get_stats, rdv_get_group_stats, rdv_eval_summary, rdv_eval_group_summary, rdv_restore,
 *   rdv_set_param_groups (they synchronise or allocate), rdv_policy_set_weights, rdv_policy_set_member_weights, rdv_lstm_set_weights
 *   and rdv_lstm_set_member_weights (their staging buffer is reused).  rdv_create,
 *   rdv_destroy and the policy create / destroy calls allocate and are not to be made while a capture is open either.
 *   SUPPORTED between replays, eagerly, on the stream that replays: rdv_step (the persistent kernels of a graph find the prepared states
 *   of the envs whose episodes it ended out of date by their tags and refill them before their first use) and rdv_set_params (it
 *   clears those tags on the device, so the next persistent launch, replayed or not, refills every one from the new parameters).
 *   The first step after rdv_set_state / rdv_restore: recorded there, a graph keeps the kRaw instantiation.  For normalised quaternions
 *   its results are bit-equal to the regular kernels', so the graph stays correct for its later replays, but it runs the in-lane layout for
 *   good: take one eager step after rdv_set_state / rdv_restore and record then.
 */
#ifndef RDV_H_
#define RDV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDV_ABI_VERSION 5
#define RDV_OBS_DIM 17    /* rendezvous_env.py:133-137 */
#define RDV_ACT_DIM 6     /* rendezvous_env.py:140-144 */
#define RDV_STATE_DIM 20  /* rc3 vc3 qc4 wc3 qt4 wt3, the column order of results/data_monte_carlo_initial_conditions.csv */
#define RDV_DIAG_DIM 8    /* pos_err, vel_err, att_err, rot_err, in_koz(now), success(now), dist_from_koz, collided(latched) */
/* (the three norms are evaluated in the order get_errors() :451-468 evaluates them under NumPy, so they are its numbers to 2 ulp also beside a
 * turned target; the flags come from the kernels' own sums of squares against the host-derived limits) */
#define RDV_EVAL_DIM 32   /* per-env evaluation accumulators, see rdv_eval_begin */

typedef enum RdvError {
  RDV_OK = 0,
  RDV_ERR_INVALID_ARGUMENT = -1,
  RDV_ERR_NO_DEVICE = -2,      /* no usable HIP device: the product path never falls back to the CPU */
  RDV_ERR_HIP = -3,            /* a HIP runtime call failed; see rdv_last_error() */
  RDV_ERR_OUT_OF_MEMORY = -4,
  RDV_ERR_BAD_HANDLE = -5,
  RDV_ERR_BAD_PARAMS = -6,     /* violates an assert of the reference ctor (rendezvous_env.py:148-156), or dt is not a multiple of 1 ms */
  RDV_ERR_DEVICE_FAULT = -7    /* a kernel of this handle reported a fault in its device error word (RdvDeviceError); the handle's
                                  results since then are not to be trusted.  Sticky: once a synchronising call (below) has read the
                                  word, every call that launches work on the handle or reads its state returns this code — rdv_reset,
                                  rdv_step, rdv_step_many, rdv_rollout, rdv_set_state, rdv_get_state, rdv_get_aux, rdv_observe,
                                  rdv_diagnose, rdv_snapshot, rdv_restore, rdv_eval_begin, rdv_eval_summary, rdv_get_stats; the
                                  parameter setters and rdv_destroy still work */
} RdvError;

/* Bits of a handle's device error word: written by the kernels (atomic OR into a word of the workspace), read back by the calls
 * that synchronise anyway (rdv_get_stats, rdv_eval_summary, rdv_restore).  Nothing a kernel detects is absorbed silently. */
typedef enum RdvDeviceError {
  RDV_DEVERR_LOST_SIGNAL = 1u  /* rdv_rollout: an env wave gave up waiting for the slot-refill signal of its workgroup (a bounded spin
                                  in LDS, ~0.3 s): it went on with slots that may be stale, so rewards / observations after that point
                                  may belong to the wrong episode */
} RdvDeviceError;

/* Precision in which the persistent per-env state is held in HBM.  Arithmetic is fp64 in both. */
typedef enum RdvStorage {
  RDV_STORAGE_F32 = 0,  /* production: 20 floats + aux per env (the 293 B/env-step layout of SURVEY §8d) */
  RDV_STORAGE_F64 = 1   /* parity mode: state held exactly as the reference holds it (NumPy float64) */
} RdvStorage;

/* What a finished episode does (SB3 DummyVecEnv auto-resets; monte_carlo.py:128 stops at done). */
typedef enum RdvOnDone {
  RDV_ON_DONE_RESET = 0,  /* in-kernel reset; obs returned is the first obs of the next episode */
  RDV_ON_DONE_HALT = 1,   /* env freezes: later steps leave it untouched and report done=1, reward=0 */
  RDV_ON_DONE_CONTINUE = 2 /* nothing happens: the env keeps stepping, as the reference's env object does when its caller ignores
                              `done` (the verification/ scripts propagate for hundreds of seconds past it); every such step
                              reports done again and counts as a finished episode in the statistics */
} RdvOnDone;

/* Which step kernel rdv_step launches.  All give the same results (same arithmetic); they differ in how the work of a
 * step is laid out on the chip.  AUTO picks SPLIT up to one 256-env workgroup per CU (n_envs <= 65536) and FUSED above. */
typedef enum RdvKernelVariant {
  RDV_VARIANT_AUTO = 0,
  RDV_VARIANT_FUSED = 1,  /* one wave does the transition of its 64 envs; the workgroup's four waves share the resets of its finished envs by part */
  RDV_VARIANT_SPLIT = 2,  /* step waves + service waves that precompute every env's next initial state beside them */
  RDV_VARIANT_FUSED_INLANE = 3, /* as FUSED, but every finished lane runs its whole reset itself (divergent); also what the evaluator
                                   build (diag / eval outputs), general rigid bodies and the first step after rdv_set_state run */
  RDV_VARIANT_FUSED_TILES = 4   /* FUSED as a tile loop: ~3 workgroups per CU walk the batch in tiles of 256 envs, the next tile's inputs
                                   requested while the current one computes (csrc/rdv_tiles.hip).  Never chosen by AUTO: measured
                                   3-8 % slower than FUSED at every size.  With on_done = HALT or a reset tape
                                   it runs FUSED */
} RdvKernelVariant;

/*
 * Environment parameters = the attributes RendezvousEnv.__init__ derives (rendezvous_env.py:52-126)
 * plus the reward_kwargs of get_bubble_reward (:313).  All doubles, no padding, 57 of them.
 * rdv_params_default() fills the reference defaults; the Python host re-derives dependent values
 * (max_axial_distance, bubble_*, n) from user kwargs exactly as the reference ctor does.
 */
typedef struct RdvParams {
  double nominal_rc0[3];        /* :52 */
  double nominal_vc0[3];        /* :53 */
  double nominal_qc0[4];        /* :54 */
  double nominal_wc0[3];        /* :55 */
  double nominal_qt0[4];        /* :56 */
  double nominal_wt0[3];        /* :57 */
  double rc0_range;             /* :60 [m]     */
  double vc0_range;             /* :61 [m/s]   */
  double qc0_range;             /* :62 [rad]   */
  double wc0_range;             /* :63 [rad/s] */
  double qt0_range;             /* :64 [rad]   */
  double wt0_range;             /* :65 [rad/s] */
  double dt;                    /* :69; a multiple of 0.001 s (dt == rint(dt*1e3)/1e3): the reference's round(t + dt, 3) (:193) follows k*dt only then, any other is refused */
  double t_max;                 /* :70 */
  double max_delta_v;           /* :81 */
  double max_delta_w;           /* :82 */
  double max_axial_distance;    /* :85 = |nominal_rc0| + 10 */
  double max_axial_speed;       /* :86 */
  double max_wc;                /* :87 */
  double max_attitude_error;    /* :89 */
  double koz_radius;            /* :93 */
  double corridor_half_angle;   /* :94 */
  double corridor_axis[3];      /* :95 target body frame */
  double capture_axis[3];       /* :73 chaser body frame */
  double rd[3];                 /* :104 target body frame */
  double max_rd_error;          /* :105 */
  double max_vd_error;          /* :106 */
  double max_qd_error;          /* :107 */
  double max_wd_error;          /* :108 */
  double bubble_radius0;        /* :114 */
  double bubble_decrease_rate;  /* :115 = 0.5*dt, per step */
  double bubble_min;            /* :116 */
  double n;                     /* :126 mean motion [rad/s] */
  double collision_coef;        /* :313 */
  double bonus_coef;            /* :313 */
  double fuel_coef;             /* :313 */
  double att_coef;              /* :313 */
} RdvParams;

/* Optional + required outputs of one step.  Nullable members are skipped when NULL. */
typedef struct RdvStepOut {
  float*   obs;             /* [N,17] required. After an auto-reset this is the reset observation (SB3 semantics) */
  float*   reward;          /* [N]    required */
  uint8_t* done;            /* [N]    required */
  float*   terminal_obs;    /* [N,17] nullable; row i written only where done[i] (SB3 info["terminal_observation"]) */
  float*   episode_return;  /* [N]    nullable; written where done (Monitor info["episode"]["r"]) */
  int32_t* episode_length;  /* [N]    nullable; written where done (Monitor info["episode"]["l"]) */
  uint8_t* done_reason;     /* [N]    nullable; bits 0-2: 0 = not done, 1 obs, 2 time, 3 bubble, 4 attitude (rendezvous_env.py:377);
                                      where done also bit 4 = the episode entered the keep-out zone, bit 5 = it had >= 1 success step */
  double*  diag;            /* [N,8]  nullable; evaluator diagnostics of the post-step (pre-reset) state, RDV_DIAG_DIM */
  double*  eval;            /* [N,32] nullable; per-env evaluation accumulators (rdv_eval_begin), updated where the env stepped */
} RdvStepOut;

/* Episode statistics accumulated on device (the list logged by custom/custom_callbacks.py:285-298): per step one
 * wavefront reduction per 64 envs into that wave's private 128-byte slot (no same-address atomics); rdv_get_stats sums
 * the slots on the host in a fixed order, so the counters are exact and the fp64 sums reproducible. */
typedef struct RdvStats {
  uint64_t env_steps;          /* env transitions executed */
  uint64_t episodes;           /* finished episodes */
  uint64_t successes;          /* finished episodes with >= 1 success step */
  uint64_t collisions;         /* finished episodes that entered the keep-out zone */
  uint64_t reasons[4];         /* termination histogram: obs, time, bubble, attitude */
  double   sum_return;         /* over finished episodes */
  double   sum_length;         /* [steps] */
  double   sum_delta_v;        /* [m/s] */
  double   sum_delta_w;        /* [rad/s] */
} RdvStats;

typedef struct RdvEnvBatch* rdv_handle;

int         rdv_version(void);
const char* rdv_last_error(void);
/* The RdvError a device error word stands for (RDV_OK for 0, RDV_ERR_DEVICE_FAULT otherwise) with the message rdv_last_error()
 * then returns naming every bit that is set.  Host-only, needs no GPU: it is the check rdv_get_stats applies to the word it reads. */
int         rdv_device_error_code(uint32_t device_error_word);
/* Test hook (ABI 4): ORs `bits` into the handle's device error word ON THE DEVICE, ordered on `stream` — exactly what a kernel that
 * detects a fault does — so that the host side of the contract (which calls read the word, which refuse afterwards) can be exercised
 * on hardware without provoking a real fault. */
int         rdv_debug_set_device_error(rdv_handle h, uint32_t bits, void* stream);
/* Test hook (ABI 5): the name of the step kernel that the last rdv_step, rdv_step_many or rdv_rollout on the handle launched, spelled
 * as its instantiation, e.g. "step_kernel_split<float, true>", "step_kernel<double, true>" (the evaluator build),
 * "step_kernel<float, false, false, true>" (the first step after rdv_set_state / rdv_restore), "step_kernel_parts<double, false>",
 * "step_kernel_tiles<float>", "step_many_kernel<float, false>", "rollout_kernel<double, false>"; "" before the first.  Recorded on
 * the host at the launch site: no device work, no synchronisation.  NULL for an invalid handle.  Static storage: do not free. */
const char* rdv_debug_last_kernel(rdv_handle h);

/* Reference ctor defaults (rendezvous_env.py:52-126, :313). Host-only, needs no GPU. */
int rdv_params_default(RdvParams* out_host);
/* The asserts of the reference ctor (:148-156) + positivity checks. Host-only. */
int rdv_params_validate(const RdvParams* params_host);

/* Bytes of device memory one batch needs (persistent SoA state + stats + parameter block + acos table + the prepared
 * next-episode state of every env that the persistent kernels rdv_step_many / rdv_rollout keep: one record and a tag). Host-only. */
int64_t rdv_workspace_bytes(int64_t n_envs, int storage);

/*
 * Create a batch of n_envs environments on `device`.  `env_id_offset` is the global index of local env 0
 * (multi-GPU sharding: RNG streams are keyed by global env id, so results do not depend on the shard count).
 * workspace: device memory of >= rdv_workspace_bytes() bytes, 256-B aligned, or NULL to let the library hipMalloc.
 * Envs are NOT initialised until rdv_reset (as RendezvousEnv: state is None until reset(), :44-49).
 */
int rdv_create(const RdvParams* params_host, int64_t n_envs, int device, int storage, int on_done,
               uint64_t seed, uint64_t env_id_offset, void* workspace, rdv_handle* out);
int rdv_destroy(rdv_handle h);

/* Replace parameters (reward coefficients, ranges, limits ...) between steps.  n/dt changes re-derive the CW matrix.
 * The new block is written by a kernel enqueued on `stream`: ordered like a step (launches already on that stream see the old
 * values, later ones the new), legal inside a stream capture, no host synchronisation.  Behind it, on `stream` too, a clear of the
 * tags of the prepared next-episode states (n_envs x 4 bytes): the persistent kernels, also those of graphs recorded earlier, then
 * refill every env's prepared state from the new block before its first use.  A change of dt inside an episode is not defined (the
 * reference keeps t across it, the library the step count): follow a set with another dt by a full rdv_reset. */
int rdv_set_params(rdv_handle h, const RdvParams* params_host, void* stream);
int rdv_get_params(rdv_handle h, RdvParams* out_host);
/* Re-key the reset RNG (VecEnv.seed()).  Episode counters restart at 0. */
int rdv_seed(rdv_handle h, uint64_t seed);

/*
 * Optional reset tape for parity tests: tape[e % depth][i][0..19] (fp64, device) is the state env i starts
 * its e-th episode from, replacing the Philox draws (the reference uses NumPy's global MT19937, which cannot
 * be replayed on device).  depth = 0 / tape = NULL returns to RNG resets.  The tape must outlive its use.
 */
int rdv_set_reset_tape(rdv_handle h, const double* tape, int32_t depth);

/* Tuning: force a kernel variant (RdvKernelVariant).  Results do not depend on it.  (Diagnostics only, read from the environment
 * at rdv_create: RDV_XCD_ORDER=0|1 forces the fused kernels' workgroup order — plain, or each XCD walking a contiguous eighth of
 * the batch, which is otherwise chosen by size; RDV_CHUNK_ALIGN / RDV_CHUNK_SKEW pad the state arrays of the workspace;
 * RDV_SPLIT_FORM=speculative|slots|slots_target|slots_target_obs forces the form of step_kernel_split<float, true> under
 * RDV_ON_DONE_RESET — the next initial state computed beside every step; prepared slots copied where an episode ends; the slot form
 * whose service waves also run the target's side of the transition and hand it to the step waves; or
 * that form with the observation and its Box test on the service waves as well (the default where it applies) — under the one
 * kernel name.) */
int rdv_set_kernel_variant(rdv_handle h, int variant);

/*
 * Rigid-body attributes of the env: self.inertia (rendezvous_env.py:75-79), self.inertia_target (:96-100) — row-major 3x3, body
 * frame — and the constant body torques handed to integrate_chaser_attitude / integrate_target_attitude (:552, :579; step()
 * passes zeros, :181, :184).  The reference constructor hard-codes 16.67 * Identity for both bodies; its right-hand side
 * (utils/dynamics.py:93-175) and its integrator (scipy solve_ivp RK45, rtol 1e-7, atol 1e-6, :561-570) are general, and the
 * attributes can be overwritten after construction.  The inverses (self.inv_inertia :80, :101) are computed by the library.
 * max_delta_w (:82, derived from inertia[0][0] in the constructor) is an RdvParams field and is not touched here.
 */
typedef enum RdvIntegrator {
  RDV_INTEGRATOR_AUTO = 0,   /* PER BODY: the closed form for a body whose tensor is c * Identity and whose torque is zero, RK45 for the
                                other (a tumbling tri-axial target beside the reference's chaser integrates the target only) */
  RDV_INTEGRATOR_EXACT = 1,  /* closed form q (x) exp(w dt / 2); refused (RDV_ERR_BAD_PARAMS) when it does not apply to both bodies */
  RDV_INTEGRATOR_RK45 = 2    /* the reference's own scheme for both bodies: Dormand-Prince 5(4) with scipy's step-size control, per env.
                                The kernel evaluates the right-hand side's two quaternion normalisations with a reciprocal square root
                                and the controller's error_norm^(-1/5) with a Newton-refined estimate (a few ulp from the reference's
                                divisions / pow): it takes scipy's accepted / rejected steps unless an error norm lies within ~1e-15
                                of 1, and lands within 1e-10 of the reference's state (tests/test_gpu_rigid_body.py) */
} RdvIntegrator;

typedef struct RdvRigidBody {
  double inertia_chaser[9];
  double inertia_target[9];
  double torque_chaser[3];
  double torque_target[3];
  double rtol;               /* :567 1e-7 */
  double atol;               /* :568 1e-6 */
  int32_t integrator;        /* RdvIntegrator */
  int32_t reserved;
} RdvRigidBody;

int rdv_rigid_body_default(RdvRigidBody* out_host);                    /* the reference constructor's values, AUTO */
int rdv_set_rigid_body(rdv_handle h, const RdvRigidBody* body_host, void* stream);   /* ordered on `stream`, like rdv_set_params */
int rdv_get_rigid_body(rdv_handle h, RdvRigidBody* out_host);

/* RendezvousEnv.reset() (:223-270) for every env, or for envs with mask[i] != 0.  obs_out [N,17] nullable. */
int rdv_reset(rdv_handle h, const uint8_t* mask, float* obs_out, void* stream);

/* RendezvousEnv.step() (:160-221) for every env: ONE kernel launch.  actions [N,6] f32 (not clipped, as :170), 8-byte aligned
 * (any row of a [K,N,6] tape is); out->obs 16-byte aligned. */
int rdv_step(rdv_handle h, const float* actions, const RdvStepOut* out_host, void* stream);

/* n_steps calls of rdv_step for an OPEN-LOOP action tape actions [n_steps,N,6] in ONE persistent launch: the env state stays in
 * registers between the steps and there is no launch boundary (~4 us per step at 65,536 envs instead of ~7.8).  out->obs
 * [n_steps,N,17], out->reward [n_steps,N], out->done [n_steps,N] and (nullable) out->done_reason [n_steps,N] are written; the
 * other members of RdvStepOut must be NULL.  Same results, final state and statistics as the loop.
 * General rigid bodies (rdv_set_rigid_body with a non-isotropic tensor, a torque, or RK45 asked for): the call runs that loop itself —
 * n_steps launches of rdv_step on `stream` (the per-lane RK45 does not fit a persistent kernel's register budget without scratch,
 * and such a step is bound by the integrator, not by launch boundaries). */
int rdv_step_many(rdv_handle h, const float* actions, int32_t n_steps, const RdvStepOut* out_host, void* stream);

/* Direct state access as monte_carlo.py:107-112 does (flags/aux are deliberately left untouched).
 * states are [N,20] fp64 row-major in CSV column order. */
int rdv_set_state(rdv_handle h, const double* states, void* stream);
int rdv_get_state(rdv_handle h, double* states_out, void* stream);
/* aux_out [N,8] fp64: t, bubble_radius, collided, success, total_delta_v, total_delta_w, episode_return, episode_index */
int rdv_get_aux(rdv_handle h, double* aux_out, void* stream);

/* Snapshot / restore of the whole batch — state, bookkeeping (t, bubble, delta-v totals, episode return), flags (collided,
 * halted, success count), episode counters (the reset RNG position) and the episode statistics — e.g. to resume an interrupted
 * evaluation or to branch rollouts from a common state.  `dst` / `src`: device buffers of rdv_snapshot_bytes(h) bytes, valid for
 * handles of the same n_envs and storage: a snapshot starts with a 64-byte header (magic, version, n_envs, storage, payload bytes)
 * that rdv_restore reads back and checks against the handle and against `src_bytes`, the size of the caller's buffer, before
 * anything is overwritten (this synchronises `stream`).  Parameters, seed and rigid bodies are not part of it.  The halted flags of
 * a snapshot mean something to handles created with RDV_ON_DONE_HALT only: restoring into a RESET or CONTINUE handle clears them, so
 * that an env restored as halted steps on there, whichever kernel steps it (rdv_step in any variant, with or without diag / eval,
 * rdv_step_many, rdv_rollout). */
int64_t rdv_snapshot_bytes(rdv_handle h);
int rdv_snapshot(rdv_handle h, void* dst, void* stream);
int rdv_restore(rdv_handle h, const void* src, int64_t src_bytes, void* stream);

/* get_observation() (:294) and the evaluator helpers (:388-468, :510) on the current state. */
int rdv_observe(rdv_handle h, float* obs_out, void* stream);
int rdv_diagnose(rdv_handle h, double* diag_out, void* stream);

/*
 * Episode-level evaluation on the device: what the reference's evaluators collect on the host after every step —
 * CustomWandbCallback.evaluate_policy (custom/custom_callbacks.py:211-267: sum of attitude errors, steps inside the keep-out zone,
 * time of the first one, smallest position error before it, total reward) and monte_carlo.evaluate (monte_carlo.py:117-205: collision
 * and success step counts, minimum distance from the KOZ, and the terminal errors of :153-189 as running sums per constraint level,
 * so that no error history is kept) — accumulated per env by rdv_step (halt mode) into `eval` [N, RDV_EVAL_DIM] fp64:
 *   0 total reward | 1 steps | 2 sum of attitude errors (k = 0 included) | 3 steps inside the KOZ | 4 time of the first one (NaN: none)
 *   5 smallest position error before it (NaN: none) | 6 success steps | 7 min dist_from_koz | 8-11 last errors (pos, vel, att, rot)
 *   then four blocks {count, sum pos, sum vel, sum att, sum rot} of the steps from the first one at which the errors met
 *   12: all four limits (:163) | 17: pos, vel and (att or rot) (:167) | 22: pos and vel (:172) | 27: pos (:175)   (strict `<`)
 * rdv_eval_begin writes the k = 0 entries from the current state (after rdv_reset / rdv_set_state, as the evaluators do);
 * rdv_eval_summary reduces the batch to the twelve means the callback logs (:285-298) with one wavefront reduction per 64 envs
 * (synchronises `stream`).
 *
 * On a RESET or CONTINUE handle rdv_step accepts `eval` too, and what it accumulates is this: every executed transition is added
 * with the diagnostics of its post-step, PRE-reset state, so the sums, counts and minima run on across episode boundaries (RESET: over
 * all the episodes an env plays; CONTINUE: over the steps past the end).  Entry 4 holds the time within the episode in which the first
 * KOZ step fell; the start state of a later episode (its k = 0 sample) is never added; a level's block never restarts.  These are
 * per-env totals over everything stepped since rdv_eval_begin, not the evaluators' per-episode records: rdv_eval_summary and
 * rdv_eval_group_summary divide by the step count of the episode an env is in (end_time / dt, 0 right after a reset), so
 * ep_collision_percentage and ep_avg_att_error are the reference's quantities in halt mode only.
 */
typedef struct RdvEvalSummary {
  double ep_rew, ep_len, ep_dist, ep_delta_v, ep_delta_w, ep_success, ep_collision_percentage;
  double ep_time_of_first_collision;   /* mean over the episodes that had one; -1 if none had (:274-277) */
  double ep_min_pos_error;             /* likewise (:279-282) */
  double ep_avg_att_error, pct_collided_episodes, pct_successful_episodes;
  int64_t episodes;
} RdvEvalSummary;
int rdv_eval_begin(rdv_handle h, double* eval, void* stream);
int rdv_eval_summary(rdv_handle h, const double* eval, RdvEvalSummary* out_host, void* stream);

/* Copy the device statistics to the host (synchronises `stream`); reset != 0 zeroes them afterwards.  Also reads the handle's device
 * error word: if a kernel set it, `out_host` is still filled and the call returns RDV_ERR_DEVICE_FAULT (sticky from then on). */
int rdv_get_stats(rdv_handle h, RdvStats* out_host, int reset, void* stream);

int64_t rdv_num_envs(rdv_handle h);

/*
 * Parameter groups (added within ABI version 5: additive exports, nothing existing changed): ONE batch, several parameter sets, ONE
 * launch per step.  The batch is divided into n_groups contiguous groups; group g covers envs [start_g, start_g + size_g), start_g
 * being the sum of the sizes in front of it, and has its own RdvParams.  What an env computes depends only on its group's
 * parameters, its global env id, the seed and its actions: it is bit for bit what a stand-alone handle of size_g envs computes that was
 * created with that group's parameters, the same seed and env_id_offset + start_g.  The use: sensitivity grids, reward tuning and
 * domain randomisation over blocks of envs without one handle, and one launch boundary per step, for every parameter set.
 *
 * The 256-env boundary rule: every group but the last must be a multiple of 256 envs, so that every group BEGINS on a multiple of 256.
 * The kernels read the parameter block with scalar loads, once per wave, and a workgroup of every step kernel owns 256 consecutive
 * envs whose finished episodes its four waves reset together from one block; a group per workgroup therefore costs one scalar
 * load (the group index of the workgroup's 256-env tile, from a table in device memory), a group boundary inside a workgroup
 * would cost the scalar parameter path.  Only the last group may end anywhere.
 *
 * rdv_param_groups_check: host-only, needs no GPU.  RDV_ERR_INVALID_ARGUMENT, with a message naming the offending group, when
 *   n_groups < 1 or there are more groups than the tile table can tell apart (one int32 index per tile, and no more groups than envs),
 *   a size is not positive, a group but the last is not a multiple of 256, or the sizes do not sum to n_envs.
 * rdv_param_groups_validate: host-only.  rdv_params_validate on each of the n_groups sets; RDV_ERR_BAD_PARAMS naming the first bad group.
 * rdv_set_param_groups: makes the handle grouped (both checks above first).  The env states are kept, as with rdv_set_params.  The
 *   G derived blocks and the tile table live in a side allocation of their own that this call makes (and frees, when a later call needs
 *   a larger one): it is the ONE group call that allocates, synchronises `stream` and is not legal inside a stream capture.  rdv_step
 *   still allocates nothing.  n_groups = 0 (the other arguments are ignored) returns the handle to its single block, the one
 *   rdv_create / rdv_set_params gave it.  A handle cannot have both groups and a general rigid body: RDV_ERR_BAD_PARAMS here on a
 *   general-body handle, and from rdv_set_rigid_body with a general body on a grouped handle.
 * rdv_set_group_params / rdv_get_group_params: one group's set.  The setter is ordered on `stream` by a kernel write, like
 *   rdv_set_params: legal inside a capture, no synchronisation.  On a grouped handle rdv_set_params and rdv_get_params are refused
 *   (RDV_ERR_INVALID_ARGUMENT, the message points here).
 * rdv_num_groups: 0 for an ungrouped handle (-1 for an invalid one).
 * rdv_get_group_stats: out_host[n_groups]; each group's statistics slots summed on the host in ascending slot order, the order
 *   rdv_get_stats of the stand-alone handle would use (counters exact, sums bit-equal).  Otherwise as rdv_get_stats, which keeps
 *   returning the whole batch.
 * rdv_eval_group_summary: rdv_eval_summary over one group's envs (rdv_eval_summary gives the whole batch, each env's times in its
 *   own group's dt).
 *
 * Which kernel runs: rdv_step launches step_kernel_groups<ST, all> (the FUSED layout with the workgroup's own block) whichever
 * RdvKernelVariant was asked for, and step_kernel_groups_lane<ST, diag, raw> for the evaluator build and the first step after
 * rdv_set_state / rdv_restore; rdv_debug_last_kernel names it.  There are no grouped persistent kernels: rdv_step_many and
 * rdv_rollout run the loop they are defined by (rdv_step, or rdv_policy_act + rdv_step, n_steps times on `stream`), as they do
 * for general rigid bodies.  rdv_reset, state access and the evaluation calls use each env's own group.  Snapshots hold no
 * parameters: rdv_restore into a grouped handle of the same n_envs and storage works as before.  A reset tape on a grouped handle is
 * indexed with the batch's n_envs and global env index.
 */
int rdv_param_groups_check(int64_t n_envs, int32_t n_groups, const int64_t* group_sizes_host);
int rdv_param_groups_validate(const RdvParams* params_host /*[n_groups]*/, int32_t n_groups);
int rdv_set_param_groups(rdv_handle h, const RdvParams* params_host /*[n_groups]*/, const int64_t* group_sizes_host, int32_t n_groups,
                         void* stream);
int rdv_set_group_params(rdv_handle h, int32_t group, const RdvParams* params_host, void* stream);
int rdv_get_group_params(rdv_handle h, int32_t group, RdvParams* out_host);
int32_t rdv_num_groups(rdv_handle h);
int rdv_get_group_stats(rdv_handle h, RdvStats* out_host /*[n_groups]*/, int reset, void* stream);
int rdv_eval_group_summary(rdv_handle h, int32_t group, const double* eval, RdvEvalSummary* out_host, void* stream);

/*
 * The actor of the reference's shipped checkpoint (SB3 MlpPolicy, 17-64-64-6, tanh; models/mlp_model_best.zip -> policy.pth,
 * built by main.py:36-46) as one kernel: actions = clip(mean(obs) [+ exp(log_std) * N(0,1)], -1, 1), the form SB3's
 * collect_rollouts / predict apply before every env.step.  Weights are HOST pointers in SB3's layout (nn.Linear [out, in]):
 * w1 [64,17], b1 [64], w2 [64,64], b2 [64], w3 [6,64], b3 [6], log_std [6].  obs [n,17] and actions [n,6] are device pointers.
 * Noise is Philox4x32-10 keyed by (seed, env_id_offset + i, counter): pass the step index as `counter`.
 *
 * The noise contract (what makes a run reproducible across shards, restarts and the two rollout forms; restated in NumPy by
 * tests/policy_reference.py and checked value by value).  For row i let id = env_id_offset + i (64 bits).  The row draws two
 * Philox4x32-10 blocks, h = 0 and h = 1, with
 *     counter words (id_lo, id_hi, counter_lo, counter_hi * 2 + h)      key (seed_lo, seed_hi ^ 0x504F4C49)
 * (lo / hi = low / high 32 bits; the key tweak keeps this stream apart from the reset stream of rdv_create's seed).  Each word w
 * becomes u = ((w >> 8) + 0.5) / 2^24 in (0, 1); each word pair (w0, w1) and (w2, w3) of a block gives two standard normals by
 * Box-Muller, (z0, z1) = sqrt(-2 ln u_first) * (cos, sin)(2 pi u_second).  Block 0 gives action components 0..3 (z0, z1 of its
 * first pair, then of its second), block 1 components 4, 5 (its first pair; its second pair is not used).  The sample is
 * mean + exp(log_std) * z, its log-density sum_c(-z_c^2 / 2 - log_std_c) - 3 ln(2 pi) is computed from z.  The kernel evaluates
 * this in fp32 with fast logarithm / sine / cosine: a normal is within 2.5e-4 of the exact value of the same words (the maximum
 * is at w >> 8 = 2^24 - 1, where the fp32 sum (w >> 8) + 0.5 rounds up, u becomes 1 and the pair is (0, 0) instead of 2^-12 (cos, sin)).
 *
 * Inputs: observations are clamped to [-63, 63] before the network (the fp16 range of the scaled operands; no effect inside the
 * observation Box [-1, 1]; +-inf counts as +-63) — the one deviation from the PyTorch modules.  A NaN in a row makes that row's six
 * actions (the critic: its value) NaN and changes no other row.  Weights must be finite; each layer's weights enter the matrix
 * cores times 2^s, s the largest integer <= 10 with max|w| * 2^s < 2^15, so one very large weight costs the small weights of
 * its layer significant bits (two fp16 terms of the scaled value).
 */
typedef struct RdvPolicyNet* rdv_policy;
int rdv_policy_create(const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host,
                      const float* w3_host, const float* b3_host, const float* log_std_host, int device, rdv_policy* out);
int rdv_policy_destroy(rdv_policy p);
int rdv_policy_act(rdv_policy p, const float* obs, float* actions, int64_t n, int deterministic, uint64_t seed,
                   uint64_t counter, uint64_t env_id_offset, void* stream);

/*
 * The critic of the same checkpoint (mlp_extractor.value_net.{0,2} [64,17], [64,64] + value_net [1,64]; SB3 MlpPolicy keeps
 * separate actor and critic trunks): values [n] for observations [n,17], e.g. for the [T*N,17] rows of a rollout (SB3's
 * compute_returns_and_advantage needs them).  Same kernel structure and accuracy as the actor.  The handle type is shared;
 * rdv_policy_destroy frees it.
 */
int rdv_critic_create(const float* w1_host, const float* b1_host, const float* w2_host, const float* b2_host,
                      const float* w3_host, const float* b3_host, int device, rdv_policy* out);
int rdv_policy_value(rdv_policy critic, const float* obs, float* values, int64_t n, void* stream);

/*
 * Other MLP architectures (added within ABI 5): what the reference's network sweep trains (tune_policy.py:30-34, :124-139:
 * net_arch = [n_neurons] * n_layers, activation_fn in {ReLU, Sigmoid, Tanh}; custom/custom_networks.py:9-10: ReLU, [32, 32]) —
 * separate actor and critic trunks of 1..4 hidden layers, each 16, 32 or 64 wide (layers may differ), ONE activation for the whole
 * network (SB3's activation_fn), 17 inputs, 6 outputs (actor) or 1 (critic).  weights_host / biases_host are arrays of n_hidden + 1
 * HOST pointers, hidden layers first, the head last, in SB3's layout (nn.Linear [out, in]): layer 0 [hidden[0], 17], layer l
 * [hidden[l], hidden[l-1]], head [6 or 1, hidden[n_hidden-1]].  The handles are rdv_policy handles: rdv_policy_act, rdv_policy_value,
 * rdv_rollout and rdv_policy_destroy take them; the noise contract, the +-63 input clamp, the NaN rule and the weight scaling above
 * hold for them unchanged, and a non-finite weight is RDV_ERR_BAD_PARAMS.  The kernels (csrc/rdv_policy_mlp.h) use the scheme of the
 * shipped actor's; a width of 64 is two 32-row MFMA tiles, 32 one, 16 one tile whose rows 16..31 have zero weights and are not
 * read by the next layer.
 *
 * Activations, in fp32 on the accumulator: tanh as above (absolute error <= 2.5e-7); sigmoid = 1 / (1 + 2^(-x log2 e)), absolute
 * error <= 2.0e-7; ReLU exact.  The second deviation from the PyTorch modules: hidden ReLU activations are clamped to [0, 63]
 * (they enter the next layer as scaled fp16 terms, as the inputs do; a NaN stays NaN).  Nothing changes for a network whose hidden
 * units stay below 63.
 *
 * With the default spec ({2, {64, 64}, RDV_ACT_TANH}) the two create calls below ARE rdv_policy_create / rdv_critic_create: the same
 * parameter block, the same kernels, bit-identical outputs, the persistent rollout kernel.  rdv_policy_get_spec works on every
 * rdv_policy handle (the default spec for handles of rdv_policy_create / rdv_critic_create).  rdv_mlp_spec_check needs no GPU and
 * names the offending field in rdv_last_error.
 */
typedef enum RdvActivation { RDV_ACT_TANH = 0, RDV_ACT_RELU = 1, RDV_ACT_SIGMOID = 2 } RdvActivation;
#define RDV_MLP_MAX_HIDDEN 4
typedef struct RdvMlpSpec {
  int32_t n_hidden;                     /* 1..4 */
  int32_t hidden[RDV_MLP_MAX_HIDDEN];   /* each 16, 32 or 64; entries from n_hidden on are 0 */
  int32_t activation;                   /* RdvActivation */
  int32_t reserved;                     /* 0 */
} RdvMlpSpec;
int rdv_mlp_spec_default(RdvMlpSpec* out_host);
int rdv_mlp_spec_check(const RdvMlpSpec* spec_host);
int rdv_policy_create_mlp(const RdvMlpSpec* spec_host, const float* const* weights_host, const float* const* biases_host,
                          const float* log_std_host, int device, rdv_policy* out);
int rdv_critic_create_mlp(const RdvMlpSpec* spec_host, const float* const* weights_host, const float* const* biases_host,
                          int device, rdv_policy* out);
int rdv_policy_get_spec(rdv_policy p, RdvMlpSpec* out_host);

/*
 * Closed-loop rollout collection in ONE launch: for t in [0, n_steps): a_t ~ actor(obs_t); obs_{t+1}, r_t, done_t =
 * step(clip(a_t)) — the inner loop of SB3's OnPolicyAlgorithm.collect_rollouts (what model.learn, main.py:114, spends its
 * env time in) with the actor above, writing the rows SB3's RolloutBuffer.add receives.  Results are those of
 * rdv_policy_act(counter = noise_counter0 + t, env_id_offset = the handle's) followed by rdv_step, n_steps times; the env
 * state stays in registers and the observations / actions in LDS in between.  Episode statistics accumulate as in rdv_step.
 * General rigid bodies (rdv_set_rigid_body with a non-isotropic tensor, a torque, or RK45 asked for): the call runs rdv_policy_act +
 * rdv_step itself, n_steps times on `stream` (2 launches per step; the one-launch form spilled and was slower than this loop).
 * A policy of another architecture than the shipped one (rdv_policy_create_mlp with a spec that is not the default): the same loop,
 * whatever the env handle; the persistent kernel's registers and LDS are laid out for 17-64-64-6 tanh.  rdv_debug_last_kernel then
 * names the step kernel the loop launched.
 */
typedef struct RdvRolloutOut {
  float*   obs;        /* [T,N,17] required: the observation the actor saw at step t (buffer.observations) */
  float*   actions;    /* [T,N,6]  required: the sampled action BEFORE clipping (buffer.actions); the env is stepped with clip(a, -1, 1) */
  float*   reward;     /* [T,N]    required */
  uint8_t* done;       /* [T,N]    required (buffer.episode_starts of step t+1) */
  float*   log_prob;   /* [T,N]    nullable: log-density of actions[t] under the actor's diagonal Gaussian (buffer.log_probs) */
  float*   last_obs;   /* [N,17]   required: the observation after the last step (SB3 _last_obs), reset observations included */
} RdvRolloutOut;
int rdv_rollout(rdv_handle h, rdv_policy p, int32_t n_steps, const RdvRolloutOut* out_host, int deterministic,
                uint64_t noise_seed, uint64_t noise_counter0, void* stream);

/*
 * Learner-ready rollouts (added within ABI 5): the columns of SB3's RolloutBuffer that rdv_rollout does not write — values, advantages,
 * returns (RolloutBuffer.compute_returns_and_advantage, called by collect_rollouts; reference main.py:114) — and the refresh of a policy
 * handle's weights after an optimiser step.  The reference never sets TimeLimit.truncated (vec_env.py:6-7), so SB3's time-limit
 * bootstrap does not apply and is not built.  The loss and the gradients of one PPO minibatch are rdv_ppo_loss_grad ("PPO minibatch
 * gradients", below); out of scope: advantage normalisation (SB3 normalises per minibatch in train(); the Python layer does it in
 * torch), gradient clipping, the optimiser and its schedules, which stay PyTorch's.
 *
 * rdv_gae: generalised advantage estimation over [T,N] rows, ONE kernel for all T steps (csrc/rdv_advantages.h).  reward, done, values,
 *   advantages and returns are [n_steps, n] contiguous device arrays, time-major, as rdv_rollout writes them; last_value is [n].  done[t]
 *   is the row of step t, SB3's episode_starts[t+1].  The contract: the outputs are BIT-IDENTICAL to SB3's loop evaluated in NumPy
 *   float32.  With g = (float)gamma and c = (float)(gamma * gae_lambda) — the product taken in double, then rounded once — for
 *   t = n_steps-1 .. 0 and each env i:
 *       nnt   = 1.0f - (float)done[t][i]
 *       nv    = (t == n_steps-1) ? last_value[i] : values[t+1][i]
 *       delta = ((reward[t][i] + (g * nv) * nnt) - values[t][i])
 *       A     = delta + ((c * nnt) * A)                     A = 0 before the first step
 *       advantages[t][i] = A;   returns[t][i] = A + values[t][i]
 *   Every operation is rounded to fp32 on its own, in exactly this association: no fused multiply-add (a * b + c contracted into an
 *   FMA rounds once where NumPy rounds twice, and changes the last bit); the kernel is compiled with contraction off.  A NaN or an
 *   infinity in a row reaches only that env's outputs.  The recurrence is not split over T (segments plus a carry fix-up re-associate
 *   the products: not bit-exact), so each env is one sequential chain: at small n the call is bound by latency, not bandwidth.
 *   RDV_ERR_INVALID_ARGUMENT, the message naming the argument, for a null pointer, n_steps <= 0, n <= 0, and a gamma or gae_lambda that
 *   is not finite or lies outside [0, 1]; these checks come before the device check and need no GPU.  The outputs must not alias the
 *   inputs (not checked).  Enqueued on `stream`, legal inside a stream capture, no allocation, no synchronisation.
 *
 * rdv_rollout_advantages: values and advantages of a rollout in one call.  On `stream`, in this order: the critic over the
 *   [n_steps * n, 17] rows of rows->obs into out->values, the critic over rows->last_obs into out->last_value — both by the launch of
 *   rdv_policy_value (shipped or general architecture: values are bit-identical to what rdv_policy_value gives for the same rows; there
 *   is no second critic kernel) — then the kernel of rdv_gae.  It reads rows->obs, rows->reward, rows->done and rows->last_obs; the
 *   other members of `rows` may be NULL.  All four members of `out` are required.  The values are the critic's AT CALL TIME for the
 *   observations the actor saw; for an env that was reset at the last step, last_obs is the reset observation, whose value is multiplied
 *   by nnt = 0, as in SB3.  Argument checks as rdv_gae's (before the handle is looked at); then RDV_ERR_BAD_HANDLE for an invalid handle,
 *   RDV_ERR_INVALID_ARGUMENT for an actor handle; alignment as rdv_policy_value (rows->obs, rows->last_obs: 16 bytes).
 *
 * rdv_policy_set_weights: new weights for an existing actor or critic handle, in the layout of rdv_policy_create_mlp: n_hidden + 1 HOST
 *   pointers each, hidden layers first, the head last; the count and the shapes are those of the handle's own spec (three layers for a
 *   handle of rdv_policy_create / rdv_critic_create).  log_std_host is required for an actor and must be NULL for a critic.  The block is
 *   packed as at creation (same size) and written into the handle's existing device allocation.  A non-finite weight is
 *   RDV_ERR_BAD_PARAMS and leaves the handle's block untouched.  ORDERING: the write is a copy enqueued on `stream` — launches already
 *   queued on that stream read the old block, launches enqueued there after this call returns read the new one, and there is no other
 *   synchronisation of the device (work on OTHER streams that uses the handle is not ordered against it: order it with events, as for any
 *   buffer).  The host arrays may be reused as soon as the call returns: they are packed into a pinned staging buffer that the handle
 *   owns (allocated by the first call), and an event recorded behind the copy makes the NEXT call on the handle wait on the host until
 *   the previous copy has left that buffer.  Because of the reused buffer it is not legal inside a stream capture
 *   (RDV_ERR_INVALID_ARGUMENT when hipStreamIsCapturing says so).
 */
typedef struct RdvAdvantageOut {
  float* values;      /* [T,N] required: critic(obs[t])      (buffer.values)     */
  float* last_value;  /* [N]   required: critic(last_obs)                        */
  float* advantages;  /* [T,N] required                      (buffer.advantages) */
  float* returns;     /* [T,N] required                      (buffer.returns)    */
} RdvAdvantageOut;
int rdv_gae(const float* reward, const uint8_t* done, const float* values, const float* last_value, int32_t n_steps, int64_t n,
            double gamma, double gae_lambda, float* advantages, float* returns, int device, void* stream);
int rdv_rollout_advantages(rdv_policy critic, const RdvRolloutOut* rows, int32_t n_steps, int64_t n, double gamma, double gae_lambda,
                           const RdvAdvantageOut* out, void* stream);
int rdv_policy_set_weights(rdv_policy p, const float* const* weights_host, const float* const* biases_host, const float* log_std_host,
                           void* stream);

/*
 * PPO minibatch gradients (added within ABI 5): the loss of SB3's PPO.train() for ONE minibatch of n samples and its gradients with respect
 * to every parameter of the shipped actor and critic, in one call on the device (csrc/rdv_ppo.h).  Gradient clipping, the optimiser (Adam)
 * and the learning-rate / clip-range schedules stay PyTorch's: they run on the gradients this call writes, and rdv_policy_set_weights then
 * pushes the new weights as before.
 *
 * The mathematics (ActorCriticPolicy.evaluate_actions with a DiagGaussianDistribution, clip_range_vf = None; eps = clip_range), for the
 * sampled rows i = 0 .. n-1, mean mu_i and value v_i of the handles' networks, sigma = exp(log_std):
 *     log_prob_i   = sum_c ( -(a_c - mu_c)^2 / (2 sigma_c^2) - log_std_c ) - 3 ln(2 pi)
 *     entropy_i    = sum_c ( 0.5 + 0.5 ln(2 pi) + log_std_c )
 *     ratio_i      = exp(log_prob_i - old_log_prob_i)
 *     policy_loss  = -mean( min(A_i ratio_i, A_i clamp(ratio_i, 1 - eps, 1 + eps)) )
 *     value_loss   = mean( (returns_i - v_i)^2 )
 *     entropy_loss = -mean( entropy_i )
 *     loss         = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 *     approx_kl    = mean( (ratio_i - 1) - (log_prob_i - old_log_prob_i) )
 *     clip_fraction = mean( |ratio_i - 1| > eps )
 *   The gradients are d loss / d theta for every actor parameter (log_std with its entropy term) and every critic parameter.  The
 *   sub-gradient of the clipped term is PyTorch's: min(x, y) passes the gradient to the strictly smaller argument and halves it between
 *   equal ones, clamp passes it inside its limits, limits included.  So d / d ratio_i of min(A ratio, A clamp(ratio)) is
 *       A_i   when 1 - eps <= ratio_i <= 1 + eps (the two arguments are equal: one half each, and the clamp passes its half), or when
 *             ratio_i lies outside and the unclipped term A_i ratio_i is the strictly smaller one;
 *       0     otherwise (outside, and the clipped term is smaller or equal).
 *   1 - eps and 1 + eps are taken in double and rounded to float once.  A comparison with a NaN is false, as in PyTorch: a NaN in any
 *   sampled row (observation, action, old_log_prob, advantage, return) reaches the gradients and the scalars — a sum has no isolation rule.
 *
 * RdvPpoRows: flat views of a rollout's rows (the [T,N,...] columns of rdv_rollout / rdv_rollout_advantages seen as [T*N,...]).  Sample i
 *   reads row indices[i] of every column, or row i when indices is NULL (then n <= rows).  The indices are NOT range-checked on the device:
 *   an index outside [0, rows) reads outside the arrays.  A duplicate index counts once per occurrence.  `advantages` holds the values as
 *   they ENTER the loss: the call never normalises.  obs must be 16-byte aligned.
 * RdvPpoOut: actor_grad [5708] = w1[64,17] b1[64] w2[64,64] b2[64] w3[6,64] b3[6] log_std[6], critic_grad [5377] = w1 b1 w2 b2 w3[1,64] b3[1],
 *   every matrix in nn.Linear's [out, in] order; scalars [8] = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, 0, 0;
 *   log_prob [n] and values [n] (both nullable): the log-density of the sampled actions under the CURRENT actor and the current critic's
 *   values, in sample order.
 *
 * The contract:
 *   - Weights: the handles' parameter blocks as of stream order — a call enqueued on `stream` after rdv_policy_set_weights on the same
 *     stream differentiates the new weights.  What is differentiated is the function the forward kernels compute: the two-term fp16
 *     weights (hi + lo) 2^-s of the block, and observations clamped to +-63.
 *   - out->values is bit-identical to what rdv_policy_value writes for the same rows, and the means inside the call are those of
 *     rdv_policy_act with deterministic = 1 before the clip: the forward half is the device code of those kernels.
 *   - Accuracy: the backward products are brought to fp32 level as the forward ones (two fp16 terms per operand, three MFMAs), the sums
 *     over rows are fp32; tests/test_gpu_ppo_grad.py holds every gradient tensor to a small multiple of the error of PyTorch's own float32
 *     autograd against an fp64 reference: err = max|G - G64| / max|G64| <= 16 max(e32, 2^-23).  Measured up to n = 1,048,576
 *     (profiles/ppo_grad_accuracy.csv): the largest err / max(e32, 2^-23) of a gradient tensor is 4.96 up to n = 549, 2.25 at n = 4,096,
 *     4.72 at n = 65,536 and 13.3 at n = 1,048,576.  The sum over the n / 256 workgroups is a float32 sum in index order, and its share
 *     grows with their number; beyond 1,048,576 samples in one call the rule has not been measured and is not claimed.
 *   - Determinism: the same inputs give the same bits in every output, eager or replayed from a captured graph.  No floating-point
 *     atomic: per-wave sums are added in wave order, per-workgroup sums go to the workspace and are added in index order.
 *   - Enqueued on `stream`, legal inside a stream capture, no allocation, no synchronisation.  The workspace is the caller's: at least
 *     rdv_ppo_workspace_bytes (n) bytes (-1 for n <= 0; needs no GPU; monotone in n), 16-byte aligned, not shared with a call in flight on
 *     another stream.  The outputs must not alias the inputs or the workspace (not checked).
 *   - Shipped architecture only: both handles 17-64-64 tanh (rdv_policy_create / rdv_critic_create or the default RdvMlpSpec), one
 *     member, not recurrent, on the same device.  rdv_ppo_spec_check judges two specs on the host (no GPU) with the messages of the call.
 *   - RDV_ERR_INVALID_ARGUMENT, the message naming the argument, for: a null rows, out or required pointer (everything but rows->indices,
 *     out->log_prob, out->values), n <= 0, rows->rows <= 0, n > rows->rows without indices, a misaligned rows->obs or workspace, a short
 *     workspace, a clip_range that is not finite or not positive, an ent_coef or vf_coef that is not finite or negative — these come
 *     before the handles are looked at and need no GPU; then RDV_ERR_BAD_HANDLE for an invalid handle; then RDV_ERR_INVALID_ARGUMENT for a
 *     recurrent handle, a policy set, actor and critic swapped, any other architecture, or handles on different devices.  A refused call
 *     enqueues nothing and leaves the handles as they were.
 */
typedef struct RdvPpoRows {          /* flat views of a rollout's [T*N] rows, device pointers */
  const float*   obs;                /* [rows,17]  16-byte aligned                          */
  const float*   actions;            /* [rows,6]   the UNCLIPPED samples (buffer.actions)   */
  const float*   old_log_prob;       /* [rows]                                              */
  const float*   advantages;         /* [rows]     as they ENTER the loss                   */
  const float*   returns;            /* [rows]                                              */
  const int64_t* indices;            /* [n] row of each minibatch sample; NULL: rows 0..n-1 */
  int64_t        rows;
} RdvPpoRows;
typedef struct RdvPpoOut {           /* device pointers */
  float* actor_grad;                 /* [5708] required */
  float* critic_grad;                /* [5377] required */
  float* scalars;                    /* [8]    required */
  float* log_prob;                   /* [n]    nullable */
  float* values;                     /* [n]    nullable */
} RdvPpoOut;
int64_t rdv_ppo_workspace_bytes(int64_t n);
int rdv_ppo_spec_check(const RdvMlpSpec* actor_spec_host, const RdvMlpSpec* critic_spec_host);
int rdv_ppo_loss_grad(rdv_policy actor, rdv_policy critic, const RdvPpoRows* rows, int64_t n, double clip_range, double ent_coef,
                      double vf_coef, void* workspace, int64_t workspace_bytes, const RdvPpoOut* out, void* stream);

/*
 * Policy sets (added within ABI 5): one batch, several actors and critics, one launch — the network half of the reference's sweeps
 * (tune_reward.py, tune_algorithm.py, tune_policy.py per architecture, the seed axis of sensitivity_analysis.py: one policy per
 * configuration), as parameter groups are the environment half.  A set is n_members networks of ONE RdvMlpSpec; member g owns
 * sizes[g] consecutive rows, member 0 from row 0 on.  The specification:
 *
 *     Row i of member g gets bit for bit what a stand-alone handle of member g's weights computes for that row, with the same
 *     seed, the same counter and env_id_offset + start_g              (start_g = sizes[0] + .. + sizes[g-1]).
 *
 * This covers the clipped action, the unclipped sample, log_prob and the value; the noise contract above keys by global env id
 * (env_id_offset + flat row of the set), so it holds as it stands.
 *
 * The 256-row rule: every size is positive and every size but the last is a multiple of 256 rows — the rule of parameter groups,
 * checked by rdv_param_groups_check (host-only), whose message names the offending member as "group".  A workgroup of the actor
 * kernels owns 256 rows and stages one parameter block; the set kernels (csrc/rdv_policy_sets.h) stage the block of their tile's
 * member and are otherwise the kernels of stand-alone handles.  The same-spec rule: all members have the spec given at creation
 * (the default spec: the shipped 17-64-64 tanh block and its kernels); members of different architectures are not offered.
 *
 * rdv_policy_set_create / rdv_critic_set_create: weights_host[g] and biases_host[g] are member g's arrays of n_hidden + 1 HOST
 *   pointers in the layout of rdv_policy_create_mlp, log_std_host[g] its [6] (actors).  Checked per member as there (null pointers:
 *   RDV_ERR_INVALID_ARGUMENT, a non-finite weight: RDV_ERR_BAD_PARAMS, the message naming layer and member), all before the device is
 *   touched.  One device allocation holds the member blocks — exactly the bytes of stand-alone handles — and the tile table.  The result
 *   is an rdv_policy: rdv_policy_destroy, rdv_policy_get_spec work on it.  n_members = 1 is legal and equals the plain handle (the plain
 *   kernels, the persistent rollout kernel), with the row checks below.
 * rdv_policy_num_members / rdv_policy_num_rows: 1 / 0 for a plain handle (-1 for an invalid one), as rdv_num_groups reports.
 * Which calls accept a set:
 *   rdv_policy_act          n must equal the set's rows (RDV_ERR_INVALID_ARGUMENT naming both numbers otherwise).
 *   rdv_policy_value        n must be a positive multiple of the set's rows: obs is [k, rows, 17], flat row r belongs to env r mod rows
 *                           (the [T, N, 17] rows of a rollout).  Row blocks whose first row is not 16-byte aligned (rows % 4 != 0) are
 *                           read element-wise: obs itself must be 16-byte aligned, as for a plain handle.
 *   rdv_rollout_advantages  passes n_steps and n through to rdv_policy_value: n must equal the set's rows.
 *   rdv_rollout             the set's rows must equal the handle's envs.  A set of more than one member takes the loop the call is
 *                           defined by (rdv_policy_act + rdv_step, n_steps times), whatever the env handle: there is no persistent
 *                           kernel for sets.  A set's ranges and the env handle's parameter groups are independent: the handle may be
 *                           ungrouped, or grouped with the same or other sizes.
 *   rdv_policy_set_weights  RDV_ERR_INVALID_ARGUMENT for a set of more than one member: use rdv_policy_set_member_weights.
 * rdv_policy_set_member_weights: rdv_policy_set_weights for ONE member (arguments, checks, ordering on `stream` and the refusal inside a
 *   stream capture as there; member 0 of a plain handle is the handle).  Launches already queued on the stream read the old block of
 *   that member, later ones the new; the other members' blocks are not written.  The pinned staging has one slot and one event per
 *   member: refreshing all members back to back does not wait on the host for another member's copy, only a second refresh of the
 *   SAME member waits for its first copy.
 */
int rdv_policy_set_create(const RdvMlpSpec* spec_host, int32_t n_members, const int64_t* sizes_host,
                          const float* const* const* weights_host, const float* const* const* biases_host,
                          const float* const* log_std_host, int device, rdv_policy* out);
int rdv_critic_set_create(const RdvMlpSpec* spec_host, int32_t n_members, const int64_t* sizes_host,
                          const float* const* const* weights_host, const float* const* const* biases_host, int device, rdv_policy* out);
int rdv_policy_set_member_weights(rdv_policy p, int32_t member, const float* const* weights_host, const float* const* biases_host,
                                  const float* log_std_host, void* stream);
int32_t rdv_policy_num_members(rdv_policy p);
int64_t rdv_policy_num_rows(rdv_policy p);

/*
 * PPO minibatch gradients for policy sets (added within ABI 5: additive exports): the minibatches of all P members of an actor set and a
 * critic set in ONE call of four launches — the update half of a sweep of P learners, as the set kernels are its rollout half.  A call
 * of rdv_ppo_loss_grad is latency-bound (one workgroup per 256 samples on a 256-CU chip); P members' minibatches are P independent sets
 * of workgroups, and here they share the launches.  The specification:
 *
 *     Every output of member g is bit for bit what rdv_ppo_loss_grad writes for stand-alone handles of member g's weights, given the
 *     same `rows`, indices + off_g, n = counts_host[g] and the same coefficients       (off_g = counts_host[0] + .. + counts_host[g-1]).
 *
 * actor_set / critic_set: handles of rdv_policy_set_create / rdv_critic_set_create with the same number of members P
 *   (rdv_policy_num_members), the default (shipped) spec, the same device.  A plain handle is a set of one member and is accepted.  The
 *   set's rows and its 256-row ranges play no part: membership of a sample is given by the counts alone.
 * counts_host [P], host: counts_host[g] >= 0 is member g's minibatch size; at least one is positive.  A member with count 0 takes no
 *   part: nothing of its gradient, scalar, log_prob or value outputs is written.
 * rows: as for rdv_ppo_loss_grad, but rows->indices is REQUIRED: a device array of off_P = sum of the counts entries, member g's samples
 *   at indices[off_g .. off_g + counts_host[g]), each a flat row of the rollout's columns.  Not range-checked on the device; a duplicate
 *   counts once per occurrence.  All members read the same columns (members of a set own different env columns of one rollout).
 * RdvPpoSetOut: actor_grad [P,5708], critic_grad [P,5377], scalars [P,8] (row g: member g's, in the layout of RdvPpoOut); log_prob and
 *   values [off_P] (both nullable), member g's at off_g.
 * One clip_range / ent_coef / vf_coef serves all members.
 *
 * Everything else of the contract of rdv_ppo_loss_grad carries over: the weights are the members' blocks as of stream order (a call
 * behind rdv_policy_set_member_weights on the same stream differentiates that member's new block, the other members are unaffected); no
 * floating-point atomic; the same bits eager or replayed from a captured graph; enqueued on `stream` only — no allocation, no
 * synchronisation, no copy, legal inside a stream capture.  The counts travel by value in the kernel arguments, which is why a call
 * serves at most 64 members (kPpoSetMaxMembers of csrc/rdv_ppo.h: 64 x 3 x 8 bytes of the 4 KiB kernel-argument segment).  The workspace
 * is the caller's: at least rdv_ppo_set_workspace_bytes (n_members, counts_host) bytes, 16-byte aligned, laid out member after member
 * as [the two backward blocks | one row of partial sums per 256 samples].  rdv_ppo_set_workspace_bytes needs no GPU, returns -1 for
 * n_members outside 1..64, null counts, a negative count or no positive one, and is monotone in every count.
 *
 * A refused call enqueues nothing and leaves both handles usable; the message names the argument.  RDV_ERR_INVALID_ARGUMENT, host-only
 * and before the handles are judged, for: a null rows, out, counts_host or required pointer (rows->indices among them; out->log_prob and
 * out->values are nullable), a negative count, no positive count, rows->rows <= 0, a misaligned rows->obs or workspace, a short
 * workspace, a clip_range that is not finite or not positive, an ent_coef or vf_coef that is not finite or negative.  (The number of
 * counts examined is actor_set's member count; with an invalid actor_set it is 1.)  Then RDV_ERR_BAD_HANDLE for an invalid handle.  Then
 * RDV_ERR_INVALID_ARGUMENT for: a recurrent handle or recurrent set, actor and critic swapped, any other architecture, different member
 * counts, more than 64 members, different devices.
 */
typedef struct RdvPpoSetOut {        /* device pointers */
  float* actor_grad;                 /* [P,5708]        required */
  float* critic_grad;                /* [P,5377]        required */
  float* scalars;                    /* [P,8]           required */
  float* log_prob;                   /* [sum of counts] nullable */
  float* values;                     /* [sum of counts] nullable */
} RdvPpoSetOut;
int64_t rdv_ppo_set_workspace_bytes(int32_t n_members, const int64_t* counts_host);
int rdv_ppo_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvPpoRows* rows, const int64_t* counts_host,
                          double clip_range, double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes,
                          const RdvPpoSetOut* out, void* stream);

/*
 * Gradient clip, Adam and weight repack for policy sets (added within ABI 5: additive exports): what follows rdv_ppo_set_loss_grad in a
 * learner's step — SB3's clip_grad_norm_ over the policy's parameters, torch.optim.Adam (no AMSGrad, no weight decay) and the refresh of the
 * forward blocks — for all P members of an actor set and a critic set in ONE call of two launches (csrc/rdv_ppo_adam.h).  The fp32 master
 * weights, the moments and the step counters are the caller's device arrays; the call reads member g's gradients, steps its parameters
 * and rewrites its two forward blocks, with no host work beyond the argument checks.  One lr / betas / eps / max_grad_norm for all members.
 *
 * RdvAdamState (device pointers, the caller's): actor_param, actor_m, actor_v [P,5708] and critic_param, critic_m, critic_v [P,5377] in
 *   the flat layout of RdvPpoOut's gradients, row g member g's, rows back to back; step [P] int64, the steps member g has taken so far;
 *   coef [P,8], written by the call.  Every ARRAY (its first row) must be 16-byte aligned, the two gradient arrays too; rows are
 *   5708 and 5377 floats apart, so a critic row is 4-byte aligned only, and the kernels read and write these arrays float by float.
 * actor_grad [P,5708], critic_grad [P,5377]: RdvPpoSetOut's (a plain handle: RdvPpoOut's).
 * active_mask: bit g set: member g takes the step.  A member whose bit is clear is INACTIVE: nothing of its rows — gradients, parameters,
 *   moments, step, blocks, coef[g] — is read or written.
 *
 * For every active member g:
 *   - Norm.  total_norm is the 2-norm of member g's 5708 + 5377 gradient entries: actor and critic form ONE norm, as
 *     clip_grad_norm_(policy.parameters()) does.  The squares are added in double in an order fixed by the index alone (no floating-point
 *     atomic), the square root is taken in double and rounded to float once.  clip_coef = min(1, float(max_grad_norm) / (total_norm + 1e-6f)),
 *     PyTorch's expression on that float norm, evaluated in double and rounded to float once (within 1 ulp of PyTorch's own float
 *     evaluation, and exactly 1 whenever that is); it is multiplied into the gradient even when it is 1.
 *   - Step coefficients.  With t = step[g] + 1: step_size = float(lr / (1 - beta1^t)) and inv_sqrt_bc2 = float(1 / sqrt(1 - beta2^t)), both
 *     computed in double.  coef[g] = total_norm, clip_coef, step_size, inv_sqrt_bc2, skipped (0 or 1), 0, 0, 0: the four floats the
 *     elementwise step actually uses, which is stated in terms of them.
 *   - Elementwise, for every entry of both nets, in float32 with every operation rounded on its own (no fused multiply-add), sqrt and the
 *     division correctly rounded:
 *         g' = g * clip_coef
 *         m  <- m + (g' - m) * (1 - beta1)
 *         v  <- v * beta2 + ((1 - beta2) * g') * g'
 *         p  <- p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))
 *     beta1, beta2, 1 - beta1, 1 - beta2 (differences taken in double) and eps are each rounded from double to float once, on the host.
 *     step[g] <- t.
 *   - Repack.  After the step, member g's forward blocks on the device — the actor's at block g of actor_set, the critic's at block g of
 *     critic_set — are the bytes that rdv_policy_create / rdv_critic_create pack from member g's new fp32 parameters: the per-layer shift
 *     (the largest s <= 10, down to -20, with max|w| 2^s < 2^15; an all-zero layer: 10), the two fp16 terms rounded to nearest even with
 *     fp16 subnormals kept, the fragment permutation, the biases in accumulator order times 2^(10 + s), log_std, the inverse scales, the
 *     zero padding.  ONE EXCEPTION: the six exp(log_std) floats of an actor block.  Host packer and device both write the
 *     double-precision exp rounded to float, but through two libraries' exp: the floats are promised within 1 ulp of each other, and are
 *     equal unless the two double results straddle a float rounding boundary (a chance of about 2^-29 per value).  (The host packer took
 *     the C library's expf before, which is not correctly rounded and differed from the device's float in about one value of a thousand.)
 *     What follows from the exception: after a device step the set sentence "row i of member g equals a stand-alone handle of member g's
 *     weights" holds by equality for the deterministic action and the value, which do not read exp(log_std); SAMPLED actions, their
 *     log_prob and rdv_ppo_set_loss_grad read it from the block, and equal those of a handle packed on the host from the same weights
 *     wherever the two floats are equal.
 *   - Non-finite gradients.  If total_norm is not finite (a NaN or an infinity among the gradients, or a norm beyond float's range),
 *     member g is skipped whole: its parameters, moments, step and blocks are untouched, coef[g] = total_norm, 0, 0, 0, 1, 0, 0, 0.  The
 *     other members are unaffected.  Parameters that leave the finite range through the step itself are NOT checked.
 *
 * The contract:
 *   - Enqueued on `stream` only: no allocation, no synchronisation, no host-device copy; legal inside a stream capture.  The step counters
 *     and the moments live in device memory, so each replay of a captured graph takes the NEXT step; lr and the other by-value arguments
 *     are those of the capture.  Launches queued earlier on the stream read the old blocks, later ones the new blocks.
 *   - Determinism: the same inputs give the same bits, eager or replayed.
 *   - The caller's side of the bargain: actor_param / critic_param must hold the weights the blocks were packed from.  The call never reads
 *     fp32 weights back out of a block; it overwrites the blocks with the pack of the stepped arrays.  The arrays must not alias one another.
 *   - Shipped architecture only (17-64-64 tanh, the default RdvMlpSpec), sets of 1..64 members; a plain handle is a set of one.  No existing
 *     call changes: rdv_policy_set_member_weights refreshes a block from host arrays as before (and knows nothing of the state arrays).
 *   - A refused call enqueues nothing; the message names the argument.  RDV_ERR_INVALID_ARGUMENT, host-only and before the handles are
 *     judged, for: a null state or pointer; a misaligned array; an lr or eps that is not finite or not positive; a beta outside [0, 1); a
 *     max_grad_norm that is not positive (+inf is legal and means no clipping); an empty mask; a mask bit at or beyond the member count (that
 *     of actor_set; with an invalid actor_set it is 1).  Then RDV_ERR_BAD_HANDLE for an invalid handle.  Then RDV_ERR_INVALID_ARGUMENT, in
 *     the order of rdv_ppo_set_loss_grad, for: a recurrent handle or set, actor and critic swapped, any other architecture, different
 *     member counts, more than 64 members, different devices.
 *
 * rdv_policy_block_floats: the floats of ONE member's parameter block of a handle (8372 for the shipped block); -1 for an invalid handle.
 * rdv_policy_get_block: block `member` of the handle, as the kernels read it, into out_host [floats] (floats must equal
 *   rdv_policy_block_floats).  A synchronous read-back for tests and checkpoints: it is ordered on `stream`, waits for it, and is refused
 *   inside a stream capture.
 */
typedef struct RdvAdamState {        /* device pointers, the caller's; every array 16-byte aligned */
  float*   actor_param;              /* [P,5708]  fp32 master weights, layout of RdvPpoOut.actor_grad  */
  float*   critic_param;             /* [P,5377]                                                       */
  float*   actor_m,  *actor_v;       /* [P,5708]  Adam moments                                         */
  float*   critic_m, *critic_v;      /* [P,5377]                                                       */
  int64_t* step;                     /* [P]       steps taken so far; the call increments an active member's */
  float*   coef;                     /* [P,8]     out: total_norm, clip_coef, step_size, inv_sqrt_bc2, skipped (0/1), 0, 0, 0 */
} RdvAdamState;
int rdv_ppo_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state,
                          const float* actor_grad, const float* critic_grad, uint64_t active_mask,
                          double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream);
int64_t rdv_policy_block_floats(rdv_policy p);
int rdv_policy_get_block(rdv_policy p, int32_t member, float* out_host, int64_t floats, void* stream);

/*
 * PPO minibatch gradients for every MLP architecture (added within ABI 5: additive exports): rdv_ppo_loss_grad for handles of ANY
 * RdvMlpSpec — 1..4 hidden layers of 16 / 32 / 64, tanh, ReLU or sigmoid, everything rdv_policy_create_mlp and rdv_critic_create_mlp
 * accept (csrc/rdv_ppo_mlp.h).  Actor and critic may differ in depth, widths and activation (SB3's net_arch = dict(pi=..., vf=...)).
 * rdv_ppo_loss_grad, rdv_ppo_spec_check, rdv_ppo_workspace_bytes and the set form are unchanged, their refusals included.
 *
 * rdv_ppo_mlp_spec_check (host-only): RDV_OK for two specs that each pass rdv_mlp_spec_check; a null pointer is
 *   RDV_ERR_INVALID_ARGUMENT naming the argument, anything else the message of rdv_mlp_spec_check behind "actor: " or "critic: ".
 * rdv_ppo_mlp_grad_floats (host-only): the length of a net's flat gradient — per layer w[out, in] then b[out], hidden layers first, the
 *   head last, every matrix in nn.Linear's [out, in] order; for an actor (is_actor != 0) log_std[6] follows.  The default spec: 5708 and
 *   5377, the layout of RdvPpoOut above.  A 16-wide layer has 16 rows: the padded rows of its tile have no entry.  -1 for a bad spec.
 * rdv_ppo_mlp_workspace_bytes (host-only): the workspace a call with handles of these specs and n samples needs; -1 for n <= 0 or a
 *   bad spec; monotone in n, a multiple of 16; for the default pair at least rdv_ppo_workspace_bytes (n).
 * rdv_ppo_mlp_loss_grad: rows, out (actor_grad and critic_grad of the lengths above), the scalars, log_prob and values as in
 *   rdv_ppo_loss_grad.
 *
 * The contract is that of rdv_ppo_loss_grad, restated for any spec:
 *   - The mathematics, PyTorch's min / clamp sub-gradient rule, the float-rounded clip limits and the NaN rule are the ones above.
 *   - What is differentiated is the function the forward kernels compute: the two-term fp16 weights of the handle's block as of stream
 *     order, observations clamped to +-63 (also in the contraction that gives the first layer's weight gradient), the bias added behind
 *     the products.  The activation's derivative is taken from the forward's own activation h: tanh 1 - h^2; sigmoid h (1 - h); ReLU 1
 *     where 0 < h < 63 and 0 elsewhere — PyTorch's 0 at the kink, and 0 where the kernel's [0, 63] cap acted.
 *   - out->values is bit-identical to what rdv_policy_value writes for the same rows, and the means inside the call are those of
 *     rdv_policy_act with deterministic = 1 before the clip: the forward half is the device code of those kernels (the hidden layers
 *     are recomputed in front of each backward step: the same code, the same bits).
 *   - Determinism: no floating-point atomic; per-wave sums in wave order, per-workgroup sums through the workspace in index order; the
 *     same bits eager or replayed from a captured graph.  A workgroup owns 256 rows, or 128 where the net's parameter block leaves
 *     the CU's LDS no room for eight waves — a function of that net's spec alone, so the bits depend on the specs and the inputs only.
 *   - Enqueue only: no allocation, no synchronisation, no host-to-device copy; legal inside a stream capture.  The workspace is the
 *     caller's, 16-byte aligned, not shared with a call in flight on another stream.
 *   - Accuracy: tests/test_gpu_ppo_mlp_grad.py holds every gradient tensor to err = max|G - G64| / max|G64| <= C max(e32, 2^-23), e32
 *     the same quantity for PyTorch's float32 autograd.  Measured (profiles/ppo_mlp_grad_accuracy.csv, n up to 549): the largest
 *     err / max(e32, 2^-23) of a gradient tensor is 8.47, at n = 1, where the lone sample's log_prob error scales every actor gradient
 *     (5.37 over n >= 33): C = 32; of a scalar 39.8: C = 128.  Larger n has not been measured under the rule for these kernels.
 *   - Handles of the default spec (the shipped block and kernels): the call IS rdv_ppo_loss_grad, its bits and, past this call's own
 *     checks, its refusals.  One default-spec handle paired with a general one is refused (RDV_ERR_INVALID_ARGUMENT).
 *   - Order of checks: first the host-only ones, RDV_ERR_INVALID_ARGUMENT naming the argument — a null rows, out or required pointer,
 *     n <= 0, rows->rows <= 0, n > rows->rows without indices, a misaligned rows->obs or workspace, the three coefficients; then
 *     RDV_ERR_BAD_HANDLE for an invalid handle; then RDV_ERR_INVALID_ARGUMENT for a recurrent handle, a policy set of more than one
 *     member, actor and critic swapped, handles on different devices, the mixed pair, and — the requirement depends on the handles'
 *     specs — a short workspace.  A refused call enqueues nothing and leaves the handles as they were.
 */
int rdv_ppo_mlp_spec_check(const RdvMlpSpec* actor_spec_host, const RdvMlpSpec* critic_spec_host);
int64_t rdv_ppo_mlp_grad_floats(const RdvMlpSpec* spec_host, int is_actor);
int64_t rdv_ppo_mlp_workspace_bytes(const RdvMlpSpec* actor_spec_host, const RdvMlpSpec* critic_spec_host, int64_t n);
int rdv_ppo_mlp_loss_grad(rdv_policy actor, rdv_policy critic, const RdvPpoRows* rows, int64_t n, double clip_range, double ent_coef,
                          double vf_coef, void* workspace, int64_t workspace_bytes, const RdvPpoOut* out, void* stream);

/*
 * PPO minibatch gradients for policy sets of every MLP architecture (added within ABI 5: additive exports): rdv_ppo_set_loss_grad for
 * an actor set and a critic set of ANY pair of RdvMlpSpec (one spec per set; csrc/rdv_ppo_mlp.h, "the set form").  The four launches of
 * rdv_ppo_mlp_loss_grad serve all P members: the member is taken from the grid, and the members' counts, offsets and workspace pieces
 * travel by value in the kernel arguments, hence the cap of 64 members.  rdv_ppo_set_loss_grad and rdv_ppo_mlp_loss_grad are unchanged.
 *
 * rdv_ppo_mlp_set_spec_check (host-only): RDV_OK for a pair of specs the call below serves; a null pointer is
 *   RDV_ERR_INVALID_ARGUMENT naming the argument, a bad spec the message of rdv_mlp_spec_check behind "actor_set: " or "critic_set: ",
 *   the mixed pair (exactly one default spec) the message of the call.
 * rdv_ppo_mlp_set_workspace_bytes (host-only): the sum of rdv_ppo_mlp_workspace_bytes (actor spec, critic spec, counts_host[g]) over
 *   the positive counts; -1 for a bad spec, n_members outside 1..64, null counts, a negative count or no positive one; monotone in every
 *   count, a multiple of 16.
 * rdv_ppo_mlp_set_loss_grad: rows, counts_host and out as in rdv_ppo_set_loss_grad; row g of out->actor_grad / out->critic_grad is
 *   rdv_ppo_mlp_grad_floats (actor spec, 1) / (critic spec, 0) floats long, the rows back to back (4-byte aligned only), in the layout
 *   of rdv_ppo_mlp_loss_grad.
 *
 * The contract, by equality: every output of member g — gradients, scalars, log_prob, values — is bit for bit what
 * rdv_ppo_mlp_loss_grad writes for stand-alone handles of member g's weights and the sets' two specs, given the same rows,
 * indices + off_g (off_g: the sum of the earlier counts), n = counts_host[g] and the same coefficients.  A member's partition into
 * workgroups (256 or 128 rows, per net), its wave order and its index-order sum are the stand-alone call's.  The rest is the contract
 * of rdv_ppo_set_loss_grad: nothing of a member with count 0 is written; one clip_range / ent_coef / vf_coef for all members; weights as
 * of stream order (a call behind rdv_policy_set_member_weights differentiates the new block); no floating-point atomic; the same bits
 * eager or replayed; enqueue only, legal inside a capture; a plain general-spec handle pair is a set of one member.
 *   - Two sets of the default spec: the call IS rdv_ppo_set_loss_grad, its bits and its refusals.  One default-spec set beside a general
 *     one is refused (RDV_ERR_INVALID_ARGUMENT).
 *   - Order of checks: the host-only ones of rdv_ppo_set_loss_grad, naming the argument, then the three coefficients; RDV_ERR_BAD_HANDLE
 *     for an invalid handle; RDV_ERR_INVALID_ARGUMENT for a recurrent handle, swapped handles, the mixed pair, different member counts,
 *     more than 64 members, two devices, and — it depends on the handles' specs — a short workspace.  A refused call enqueues nothing.
 */
int rdv_ppo_mlp_set_spec_check(const RdvMlpSpec* actor_spec_host, const RdvMlpSpec* critic_spec_host);
int64_t rdv_ppo_mlp_set_workspace_bytes(const RdvMlpSpec* actor_spec_host, const RdvMlpSpec* critic_spec_host, int32_t n_members,
                                        const int64_t* counts_host);
int rdv_ppo_mlp_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvPpoRows* rows, const int64_t* counts_host,
                              double clip_range, double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes,
                              const RdvPpoSetOut* out, void* stream);

/*
 * Gradient clip, Adam and weight repack for policy sets of every MLP architecture (added within ABI 5: additive export):
 * rdv_ppo_set_adam_step for an actor set and a critic set of ANY pair of RdvMlpSpec (csrc/rdv_ppo_adam.h, "every MLP architecture"),
 * what follows rdv_ppo_mlp_set_loss_grad in a sweep's update step.  RdvAdamState is reused as it is; its rows, and those of actor_grad /
 * critic_grad, are Ga = rdv_ppo_mlp_grad_floats (actor spec, 1) and Gc = rdv_ppo_mlp_grad_floats (critic spec, 0) floats long, back to
 * back, in the layout of rdv_ppo_mlp_loss_grad (the base pointers 16-byte aligned, the rows 4-byte aligned only).
 *
 * The contract is that of rdv_ppo_set_adam_step, restated for any pair of specs:
 *   - One norm per member over its Ga + Gc entries: squares added in double (thread t adds entries t, t + 256, .. of [actor | critic],
 *     then a fixed tree), the square root in double rounded to float once; clip_coef, the two step coefficients, coef[g] and step[g] as
 *     in rdv_ppo_set_adam_step; a member whose norm is not finite is skipped whole (coef[g][4] = 1).
 *   - The elementwise step: the same four float32 lines, every operation rounded on its own.
 *   - Member g's two forward blocks become the bytes pack_mlp_weights (what rdv_policy_create_mlp / rdv_critic_create_mlp pack) gives from
 *     the new fp32 parameters — the per-layer shift, the two fp16 terms rounded to nearest even with subnormals kept, the fragment order,
 *     zero fragments for the rows and k-steps a 16- or 32-wide layer does not have, the head's rows >= out_dim zero, the biases in
 *     accumulator order, each layer's inverse accumulator scale, log_std — but for the six exp(log_std) floats of an actor block: the
 *     double-precision exp rounded to float, within 1 ulp of the host's.
 *   - Two launches, no workspace, nothing read back from a block; a member whose mask bit is clear has nothing read or written; no
 *     floating-point atomic; the same bits eager or replayed; enqueue only, legal inside a capture (each replay takes the next step).
 *   - Two sets of the default spec: the call IS rdv_ppo_set_adam_step, its bits and its refusals.  One default-spec set beside a general
 *     one is refused.  Order of checks and messages: those of rdv_ppo_set_adam_step (host-only checks naming the argument, then
 *     RDV_ERR_BAD_HANDLE, then recurrent / swapped / the mixed pair / member counts / more than 64 members / two devices).
 */
int rdv_ppo_mlp_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state,
                              const float* actor_grad, const float* critic_grad, uint64_t active_mask,
                              double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream);

/*
 * The recurrent policy (added within ABI 5: additive exports): what the reference's main_rnn.py trains and tune_policy.py:80, :140-148
 * and tune_algorithm.py:68 build — sb3-contrib RecurrentPPO("MlpLstmPolicy"), i.e. RecurrentActorCriticPolicy with ONE LSTM layer of
 * lstm_hidden_size H in front of the mlp_extractor trunk, and separate LSTMs for actor and critic (shared_lstm = False,
 * enable_critic_lstm = True, the defaults).  Per env row, with obs x [17], state (h, c) [H] each and episode_start s in {0, 1}:
 *
 *     h, c   <- (1 - s) h, (1 - s) c
 *     a      =  W_ih x + b_ih + W_hh h + b_hh            W_ih [4H, 17], W_hh [4H, H], gate rows in torch.nn.LSTM's order i, f, g, o
 *     c'     =  sigmoid(a_f) c + sigmoid(a_i) tanh(a_g)
 *     h'     =  sigmoid(a_o) tanh(c')
 *     latent =  h'  ->  trunk (an RdvMlpSpec: 1..4 hidden layers of 16 / 32 / 64, one activation; its first layer is [hidden[0], H])
 *     actor:  mean = action_net(latent) [6]; sample, clip and log_prob exactly as rdv_policy_act (the noise contract above, unchanged)
 *     critic: value = value_net(latent) [1], from ITS OWN LSTM and trunk
 *
 * What is served: H in {32, 64, 128, 256} (tune_policy.py's axis), n_layers = 1, shared = 0.  Refused by name with RDV_ERR_BAD_PARAMS
 * (rdv_lstm_spec_check, host-only, needs no GPU, the message names the field): any other hidden_size, n_layers != 1 (more LSTM layers),
 * shared != 0 (a shared LSTM; a critic without an LSTM of its own is the same refusal: every critic handle here has one), reserved != 0;
 * the trunk is judged by rdv_mlp_spec_check.  The +-63 input clamp, the NaN rule (a NaN in a row reaches that row's outputs and that
 * row's state, no other row) and the weight scaling of the MLP kernels hold: W_ih and W_hh share one power-of-two scale; a non-finite
 * weight is RDV_ERR_BAD_PARAMS.  The state enters the matrix cores as the inputs do (times 2^10, two fp16 terms, clamped to +-63: no
 * effect on a state the cell produced, |h| < 1).  Kernels: csrc/rdv_policy_lstm.h — two launches per call, the cell and the trunk.
 *
 * rdv_lstm_policy_create / rdv_lstm_critic_create: arrays are HOST pointers in torch's layout — w_ih [4H, 17], w_hh [4H, H], b_ih, b_hh
 *   [4H]; trunk weights / biases: n_hidden + 1 pointers, hidden layers first, the head ([6 or 1, hidden[n_hidden-1]]) last; log_std [6].
 *   n_rows > 0: the rows (envs) whose state the handle owns — fp32 (h, c) [n_rows, H] each in device memory.  The result is an rdv_policy:
 *   rdv_policy_destroy frees it, rdv_policy_get_spec returns the TRUNK's spec, rdv_policy_num_rows n_rows.  The state is zero and every
 *   row's PENDING episode-start flag is 1.  The pending flags are what rdv_rollout and rdv_rollout_advantages use for their first step; a
 *   committing rdv_lstm_act / rdv_lstm_value and rdv_lstm_set_state clear them (the state then IS the caller's), rdv_rollout and
 *   rdv_rollout_advantages leave done[T-1] there.
 * rdv_lstm_act: one step of the actor for all rows.  n must equal the handle's rows.  episode_start: u8 [n] on the device, NULL = no row
 *   starts an episode.  actions [n, 6] clipped; raw_actions [n, 6] (nullable) the sample before clipping, log_prob [n] (nullable) its
 *   log-density.  Advances the state.  obs and actions 16-byte aligned.  Only enqueues on `stream`: no allocation, no synchronisation.
 * rdv_lstm_value: one step of the critic; commit = 0 evaluates without writing the state (sb3-contrib's predict_values for the value of
 *   the last observation), commit != 0 advances it.
 * rdv_lstm_get_state / rdv_lstm_set_state: h and c as [rows, H] fp32 DEVICE arrays in plain row-major order (copies on `stream`).
 * rdv_lstm_reset_state: zero state for the rows whose mask byte (u8 [rows], device) is not 0; NULL = every row.  Pending flags untouched.
 * rdv_lstm_set_weights: new weights in the layout of the create calls (log_std required for an actor, NULL for a critic); the state is
 *   kept.  Ordering on `stream`, the pinned staging buffer and the refusal inside a stream capture are rdv_policy_set_weights'.
 * rdv_lstm_hidden_size: H (-1 for an invalid handle, 0 for a handle that is not recurrent).
 *
 * Which other calls take a recurrent handle:
 *   rdv_rollout             an LSTM actor whose rows equal the handle's envs: the loop the call is defined by — rdv_lstm_act, then rdv_step,
 *                           n_steps times on `stream`.  Step 0 uses the pending flags, step t out->done[t-1]; behind the last step
 *                           out->done[T-1] is copied into the pending flags (device to device on `stream`), so the next rollout goes on
 *                           where this one stopped.  rdv_debug_last_kernel names the step kernel, as for the other loop forms.
 *   rdv_rollout_advantages  an LSTM critic whose rows equal n: n_steps COMMITTING rdv_lstm_value calls in time order over rows->obs[t] with
 *                           the same flags (pending, then rows->done[t-1]), one non-committing call on rows->last_obs with done[T-1] for
 *                           out->last_value, done[T-1] into the critic's pending flags, then the kernel of rdv_gae, unchanged.  When n % 4
 *                           != 0, row t of rows->obs is not 16-byte aligned and is read through a copy in the handle's scratch rows.
 *   rdv_policy_act, rdv_policy_value, rdv_policy_set_weights, rdv_policy_set_member_weights: RDV_ERR_INVALID_ARGUMENT (they would ignore
 *                           the state); rdv_policy_set_create builds from weights of ONE RdvMlpSpec and has no recurrent members:
 *                           recurrent networks go into a recurrent set of their own (below).
 *
 * Recurrent policy sets (added within ABI 5: additive exports) — the network half of a sweep of P recurrent learners, as policy sets
 * are for MLP learners: n_members recurrent networks of ONE RdvLstmSpec (the same H, the same trunk spec), member g owning sizes[g]
 * consecutive rows, member 0 from row 0 on.  The set handle owns the state (h, c) [rows, H] and the pending flags of all rows,
 * rows = sum(sizes).  The contract:
 *
 *     Row i of member g gets bit for bit what a stand-alone rdv_lstm_policy_create / rdv_lstm_critic_create handle of member g's arrays
 *     with n_rows = sizes[g] computes for that row, fed the same observations and episode-start flags, the same seed, the same counter
 *     and env_id_offset + start_g (start_g = sizes[0] + .. + sizes[g-1]), over any number of steps.
 *
 * This covers the clipped action, the unclipped sample, log_prob, the value, and h and c after every call (the set's state rows
 * start_g .. start_g + sizes[g] - 1 equal the stand-alone handle's state).  The 256-row rule of policy sets holds (every size positive,
 * every size but the last a multiple of 256; rdv_param_groups_check, whose message names the member as "group"): a workgroup of the
 * cell and trunk kernels owns 256 consecutive rows, so it never spans two members; the set forms of the kernels read the block of
 * their tile's member and are otherwise the kernels of stand-alone handles (csrc/rdv_policy_lstm.h).
 *
 * rdv_lstm_policy_set_create / rdv_lstm_critic_set_create: w_ih_host[g] .. b_hh_host[g], weights_host[g], biases_host[g] and (actors)
 *   log_std_host[g] are member g's arrays in the layout of rdv_lstm_policy_create.  Checked in this order, all before the device is
 *   touched: the spec (rdv_lstm_spec_check), the sizes (rdv_param_groups_check; at most 2^31 rows), every member's arrays as
 *   rdv_lstm_policy_create checks them, the message naming the member.  One device allocation holds the member blocks — exactly the
 *   bytes of stand-alone handles — and the tile table; one state allocation serves all rows.  The state is zero and every row's pending
 *   flag is 1.  n_members = 1 is legal: it runs the plain kernels and equals the plain handle.
 * Calls that take a recurrent set as they take a recurrent handle, n being the set's rows, their semantics (the pending-flag rules
 *   included) unchanged: rdv_lstm_act, rdv_lstm_value (commit 0 / 1), rdv_lstm_get_state, rdv_lstm_set_state, rdv_lstm_reset_state,
 *   rdv_lstm_hidden_size, rdv_policy_num_members, rdv_policy_num_rows, rdv_policy_get_spec, rdv_policy_destroy, rdv_rollout (the
 *   rdv_lstm_act + rdv_step loop, whatever the env handle's grouping: the set's ranges and the handle's parameter groups are independent)
 *   and rdv_rollout_advantages (as for a recurrent critic, the copy through the scratch rows when n % 4 != 0 included).
 * rdv_lstm_set_weights: RDV_ERR_INVALID_ARGUMENT for a set of more than one member: use rdv_lstm_set_member_weights.
 * rdv_lstm_set_member_weights: rdv_lstm_set_weights for ONE member (arguments, checks, ordering on `stream`, the per-member staging slot
 *   and event, and the refusal inside a stream capture as there and as rdv_policy_set_member_weights; member 0 of a plain recurrent handle
 *   is the handle).  The state and the other members' blocks are not written.
 * Not offered: a persistent one-launch recurrent rollout, 2 or 3 LSTM layers, a shared LSTM, members of different H or trunks in one
 * recurrent set, recurrent and MLP members in one set.
 */
typedef struct RdvLstmSpec {
  int32_t hidden_size;   /* 32, 64, 128 or 256 */
  int32_t n_layers;      /* 1 */
  int32_t shared;        /* 0: separate actor and critic LSTMs */
  int32_t reserved;      /* 0 */
  RdvMlpSpec trunk;
} RdvLstmSpec;
int rdv_lstm_spec_check(const RdvLstmSpec* spec_host);
int rdv_lstm_policy_create(const RdvLstmSpec* spec_host, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host,
                           const float* b_hh_host, const float* const* weights_host, const float* const* biases_host,
                           const float* log_std_host, int64_t n_rows, int device, rdv_policy* out);
int rdv_lstm_critic_create(const RdvLstmSpec* spec_host, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host,
                           const float* b_hh_host, const float* const* weights_host, const float* const* biases_host, int64_t n_rows,
                           int device, rdv_policy* out);
int rdv_lstm_act(rdv_policy p, const float* obs, const uint8_t* episode_start, float* actions, float* raw_actions, float* log_prob,
                 int64_t n, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, void* stream);
int rdv_lstm_value(rdv_policy critic, const float* obs, const uint8_t* episode_start, float* values, int64_t n, int commit, void* stream);
int rdv_lstm_get_state(rdv_policy p, float* h_out, float* c_out, void* stream);
int rdv_lstm_set_state(rdv_policy p, const float* h, const float* c, void* stream);
int rdv_lstm_reset_state(rdv_policy p, const uint8_t* mask, void* stream);
int rdv_lstm_set_weights(rdv_policy p, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host, const float* b_hh_host,
                         const float* const* weights_host, const float* const* biases_host, const float* log_std_host, void* stream);
int32_t rdv_lstm_hidden_size(rdv_policy p);
int rdv_lstm_policy_set_create(const RdvLstmSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* w_ih_host,
                               const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host,
                               const float* const* const* weights_host, const float* const* const* biases_host,
                               const float* const* log_std_host, int device, rdv_policy* out);
int rdv_lstm_critic_set_create(const RdvLstmSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* w_ih_host,
                               const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host,
                               const float* const* const* weights_host, const float* const* const* biases_host, int device,
                               rdv_policy* out);
int rdv_lstm_set_member_weights(rdv_policy p, int32_t member, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host,
                                const float* b_hh_host, const float* const* weights_host, const float* const* biases_host,
                                const float* log_std_host, void* stream);

/*
 * Recurrent PPO minibatch gradients (added within ABI 5: additive exports): the loss of SB3's PPO.train() for one minibatch of a
 * recurrent rollout and its gradients for every parameter of a stand-alone recurrent actor and critic — LSTM and trunk of each —
 * back-propagated through time in hand-written HIP (csrc/rdv_ppo_lstm.h).  It is what sb3-contrib's RecurrentPPO.train() computes for a
 * minibatch that RecurrentRolloutBuffer cuts on env boundaries: B whole env columns of a [T, N] rollout, all T steps of each, so the loss
 * means run over the n = T B entries (t, b) and nothing is padded.
 *
 * The function.  For column b (env e = envs[b], or b when envs is NULL), actor and critic each with an LSTM, a trunk and an (h0, c0) of
 * their own:
 *     (h, c)_{-1} = state0[e]        the state as step 0 of the rollout saw it — zero where an episode start was pending
 *                                    (LstmPolicy.state_at_start); a constant of the minibatch: no gradient flows into it
 *     s_t         = 0 for t = 0 (state0 is already zeroed), else done[t-1, e]
 *     (h, c)     <- (1 - s_t) (h, c)_{t-1};   a = W_ih x_t + b_ih + W_hh h + b_hh            x_t = obs[t, e]
 *     c_t         = sig(a_f) c + sig(a_i) tanh(a_g);   h_t = sig(a_o) tanh(c_t);   h_t -> trunk -> mean_t [6] / value_t
 *   The loss is the expression of rdv_ppo_loss_grad above over the rows (t, b), with its log_prob, entropy, ratio, policy_loss,
 *   value_loss, entropy_loss, approx_kl and clip_fraction, PyTorch's min / clamp sub-gradient rule, the float-rounded clip limits,
 *   clip_range_vf = None and the NaN rule (a NaN in a sampled row reaches the gradients and the scalars).
 *   Gradients: the recurrence carries them back in time; an episode start cuts them — nothing flows from step t into step t - 1 when
 *   done[t-1, e] = 1, and such a step adds nothing to dW_hh through h_{t-1}; nothing flows into state0; b_ih and b_hh get the same
 *   gradient.  What is differentiated is the function the forward kernels compute: the two-term fp16 weights of the handles' blocks as
 *   of stream order, observations clamped to +-63 (also in the contraction that gives dW_ih), h_{t-1} as the cell reads it, biases added
 *   behind the products, the trunk's activation derivatives taken from the forward's own activations (csrc/rdv_ppo_mlp.h), the cell's
 *   from its own gate activations.
 *
 * rdv_lstm_ppo_spec_check (host only): each spec judged by rdv_lstm_spec_check, its message behind "actor: " / "critic: "; then both must
 *   have the same hidden_size (RDV_ERR_INVALID_ARGUMENT).  Trunks may differ.
 * rdv_lstm_ppo_grad_floats (host only): the length of a net's flat gradient, -1 for a bad spec.  The layout: w_ih[4H,17] w_hh[4H,H]
 *   b_ih[4H] b_hh[4H] (nn.LSTM's arrays, gate order i, f, g, o), then the trunk as rdv_ppo_mlp_grad_floats lays a net out with layer 0 =
 *   [hidden[0], H] (per layer w[out, in] then b[out], the head last), log_std[6] last for an actor.
 * rdv_lstm_ppo_workspace_bytes (host only): -1 for a bad pair of specs or n_steps or n_seq <= 0; monotone in both sizes; a multiple of 16.
 *   Per row (t, b) and net the workspace keeps h_t, c_t, the four gate activations (later d loss / d a_t in their place) and
 *   d loss / d h_t: 28 H bytes (csrc/rdv_ppo_lstm.h says why the gates are kept and not recomputed).
 * RdvLstmPpoRows: device pointers.  obs [T,N,17], actions [T,N,6] (the UNCLIPPED samples), old_log_prob, advantages (as they ENTER the
 *   loss: the call never normalises), returns [T,N], done [T,N] uint8, actor_h0, actor_c0, critic_h0, critic_c0 [N,H]; envs [n_seq] int64,
 *   nullable: the columns (NULL: columns 0 .. n_seq-1, then n_seq <= n_envs); not range-checked on the device: an entry outside
 *   [0, n_envs) reads outside the arrays; a duplicate counts once per occurrence.  n_envs = N, n_steps = T, n_seq = B.  No array needs
 *   more than its element's alignment: the columns are gathered into the workspace, which must be 16-byte aligned.
 * RdvLstmPpoOut: actor_grad, critic_grad (rdv_lstm_ppo_grad_floats floats each), scalars [8] in the order of RdvPpoOut; log_prob and
 *   values [T, n_seq] (both nullable): entry (t, b) is the log-density of actions[t, e] under the CURRENT actor and the current critic's
 *   value.
 *
 * The contract:
 *   - Enqueue only: no allocation, no synchronisation, no host-to-device copy; legal inside a stream capture.  4 T + 8 launches, fixed by
 *     the specs, T and n_seq: three (gather, the two transposes), per net T cell steps, one trunk kernel, T backward steps and one
 *     weight-gradient kernel, and one finishing kernel.
 *   - Deterministic: the same inputs give the same bits in every output, eager or replayed from a captured graph.  No floating-point
 *     atomic: per-wave sums are added in wave order, per-workgroup sums go through the workspace and are added in index order.
 *   - Handles: their state and pending flags are neither read nor written; the weights are the blocks as of stream order (a call behind
 *     rdv_lstm_set_weights on the same stream differentiates the new weights).  The forward half restates the rollout's cell and trunk operation for operation: with
 *     unchanged weights out->values equals, bit for bit, what rdv_rollout_advantages wrote for those columns.
 *   - Accuracy: tests/test_gpu_ppo_lstm_grad.py holds every gradient tensor to err = max|G - G64| / max|G64| <= 32 max(e32, 2^-23) and
 *     every scalar to 128 max(e32, 2^-23), e32 the error of PyTorch's own float32 autograd against an fp64 reference on the same case;
 *     profiles/lstm_ppo_grad_accuracy.csv holds the measured ratios.
 *   - Order of checks.  Host only, the message naming the argument, RDV_ERR_INVALID_ARGUMENT: a null rows, out or required pointer
 *     (everything but rows->envs, out->log_prob, out->values), n_envs, n_steps or n_seq <= 0, n_seq > n_envs without envs, more than 2^31
 *     rows, a misaligned workspace, a clip_range that is not finite or not positive, an ent_coef or vf_coef that is not finite or
 *     negative.  Then RDV_ERR_BAD_HANDLE for an invalid handle.  Then RDV_ERR_INVALID_ARGUMENT for a handle that is not recurrent, a
 *     recurrent set of more than one member, actor and critic swapped, different hidden sizes, different devices, a short workspace.
 *     A refused call enqueues nothing and leaves the handles as they were.
 *   - The existing rdv_ppo_* calls keep refusing a recurrent handle.
 * Recurrent sets have a call of their own, rdv_lstm_ppo_set_loss_grad below (this call keeps refusing a set of more than one member).
 * The optimiser half of the step is rdv_lstm_ppo_set_adam_step at the end of this header (a plain handle pair is a set of one member).
 * Not in this call: minibatches that start mid-column from stored states, clip_range_vf, one persistent launch.
 */
typedef struct RdvLstmPpoRows {      /* device pointers: the [T,N,...] columns of a recurrent rollout */
  const float*   obs;                /* [T,N,17]                                            */
  const float*   actions;            /* [T,N,6]  the UNCLIPPED samples                      */
  const float*   old_log_prob;       /* [T,N]                                               */
  const float*   advantages;         /* [T,N]    as they ENTER the loss                     */
  const float*   returns;            /* [T,N]                                               */
  const uint8_t* done;               /* [T,N]                                               */
  const float*   actor_h0;           /* [N,H]    the actor's state as step 0 saw it         */
  const float*   actor_c0;           /* [N,H]                                               */
  const float*   critic_h0;          /* [N,H]    the critic's                               */
  const float*   critic_c0;          /* [N,H]                                               */
  const int64_t* envs;               /* [n_seq]  the minibatch's columns; NULL: 0..n_seq-1  */
  int64_t        n_envs, n_steps, n_seq;
} RdvLstmPpoRows;
typedef struct RdvLstmPpoOut {       /* device pointers */
  float* actor_grad;                 /* [rdv_lstm_ppo_grad_floats(actor spec, 1)]  required */
  float* critic_grad;                /* [rdv_lstm_ppo_grad_floats(critic spec, 0)] required */
  float* scalars;                    /* [8]          required */
  float* log_prob;                   /* [T, n_seq]   nullable */
  float* values;                     /* [T, n_seq]   nullable */
} RdvLstmPpoOut;
int rdv_lstm_ppo_spec_check(const RdvLstmSpec* actor_spec_host, const RdvLstmSpec* critic_spec_host);
int64_t rdv_lstm_ppo_grad_floats(const RdvLstmSpec* spec_host, int is_actor);
int64_t rdv_lstm_ppo_workspace_bytes(const RdvLstmSpec* actor_spec_host, const RdvLstmSpec* critic_spec_host, int64_t n_steps, int64_t n_seq);
int rdv_lstm_ppo_loss_grad(rdv_policy actor, rdv_policy critic, const RdvLstmPpoRows* rows, double clip_range, double ent_coef,
                           double vf_coef, void* workspace, int64_t workspace_bytes, const RdvLstmPpoOut* out, void* stream);

/*
 * Recurrent PPO minibatch gradients for recurrent sets (added within ABI 5: additive exports): the call above for every member of a
 * recurrent set (rdv_lstm_policy_set_create / rdv_lstm_critic_set_create) at once — the members' minibatches of whole env columns share
 * the launches (csrc/rdv_ppo_lstm.h, "the set form").
 *
 * Specification, by equality (the rule of rdv_ppo_set_loss_grad and rdv_ppo_mlp_set_loss_grad): every output of member g — both flat
 * gradients, the eight scalars, log_prob, values — is bit for bit what rdv_lstm_ppo_loss_grad writes for stand-alone handles holding
 * member g's weights, the same [T, N] columns and state0 arrays, envs + off_g, n_seq = counts[g] and the same coefficients, off_g the sum
 * of the earlier counts.  Each member keeps the stand-alone call's partition into waves and workgroups, its wave_scale values, its
 * lstm_ppo_splits(T B_g) and its wave-order and index-order sums; accuracy against fp64 is the stand-alone call's.
 *
 * rdv_lstm_ppo_set_workspace_bytes (host only): the sum of rdv_lstm_ppo_workspace_bytes(actor_spec, critic_spec, n_steps, counts_host[g])
 *   over the positive counts; -1 for a bad pair of specs, n_steps <= 0, n_members outside 1..64, null counts, a negative count or no
 *   positive count.  Monotone in every count; a multiple of 16.
 * rdv_lstm_ppo_set_loss_grad:
 *   actor_set, critic_set: recurrent sets of the same member count P <= 64, the same hidden size and the same device; a plain recurrent
 *     handle pair is a set of one member.  The sets' row ranges play no part: membership of a column is given by the counts alone.
 *   counts_host [P] (host): counts_host[g] >= 0 is B_g, member g's number of columns; at least one is positive.  Nothing of a member
 *     with count 0 is written: no gradient row, no scalars, no log_prob, no values.
 *   rows: RdvLstmPpoRows as above, but rows->envs is REQUIRED — a device array of sum B_g entries, member g's at off_g — and
 *     rows->n_seq must equal sum B_g.  The state0 arrays are the set's [N, H], shared by all members.
 *   RdvLstmPpoSetOut: actor_grad [P, Ga], critic_grad [P, Gc] (Ga, Gc: rdv_lstm_ppo_grad_floats; the rows lie back to back), scalars
 *     [P, 8]; log_prob and values (nullable): member g's [T, B_g] block is contiguous at float offset T off_g.
 * The contract is the stand-alone call's:
 *   - Enqueue only: no allocation, no synchronisation, no host-to-device copy (count, off and the workspace start of every member
 *     travel by value in the kernel arguments: hence the cap of 64); legal inside a stream capture.  4 T + 8 launches WHATEVER P: each is
 *     the stand-alone launch over the widest member's grid times the members.
 *   - Deterministic, no floating-point atomic, the same bits eager or replayed.
 *   - Handles: state and pending flags neither read nor written; weights as of stream order, so a call behind
 *     rdv_lstm_set_member_weights differentiates that member's new block and no other member's bits move.
 *   - One clip_range / ent_coef / vf_coef for all members.
 *   - Order of checks.  Host only, the message naming the argument, RDV_ERR_INVALID_ARGUMENT: a null rows, out, counts_host or required
 *     pointer (rows->envs among them; everything but out->log_prob, out->values), a negative count or none positive, rows->n_seq != the
 *     sum of the counts, n_envs or n_steps <= 0, more than 2^31 rows in a member, a misaligned workspace, the coefficients.  (counts_host
 *     is read for the actor set's members, at most 64; one entry with an invalid handle.)  Then RDV_ERR_BAD_HANDLE.  Then
 *     RDV_ERR_INVALID_ARGUMENT for a handle that is not recurrent, swapped sets, different member counts, more than 64 members,
 *     different hidden sizes, different devices, a short workspace.  A refused call enqueues nothing.
 */
typedef struct RdvLstmPpoSetOut {    /* device pointers */
  float* actor_grad;                 /* [P, rdv_lstm_ppo_grad_floats(actor spec, 1)]  required */
  float* critic_grad;                /* [P, rdv_lstm_ppo_grad_floats(critic spec, 0)] required */
  float* scalars;                    /* [P, 8]       required */
  float* log_prob;                   /* [T sum B_g]  nullable: member g's [T, B_g] at T off_g */
  float* values;                     /* [T sum B_g]  nullable */
} RdvLstmPpoSetOut;
int64_t rdv_lstm_ppo_set_workspace_bytes(const RdvLstmSpec* actor_spec_host, const RdvLstmSpec* critic_spec_host, int64_t n_steps,
                                         int32_t n_members, const int64_t* counts_host);
int rdv_lstm_ppo_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvLstmPpoRows* rows, const int64_t* counts_host,
                               double clip_range, double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes,
                               const RdvLstmPpoSetOut* out, void* stream);

/*
 * Gradient clip, Adam and weight repack for recurrent policy sets (added within ABI 5: additive exports): rdv_ppo_set_adam_step for a
 * recurrent actor set and a recurrent critic set — what follows rdv_lstm_ppo_set_loss_grad (or rdv_lstm_ppo_loss_grad) in a learner's
 * step, for all P members in ONE call of FOUR launches, fixed by nothing but the call itself: the same four whatever P, H and the trunks
 * (csrc/rdv_ppo_lstm_adam.h).  A plain recurrent handle pair is a set of one member.  rdv_ppo_set_adam_step and rdv_ppo_mlp_set_adam_step
 * keep refusing recurrent handles.
 *
 * RdvAdamState as above, with rows of Ga = rdv_lstm_ppo_grad_floats(actor spec, 1) and Gc = rdv_lstm_ppo_grad_floats(critic spec, 0)
 * floats, back to back, in the layout of rdv_lstm_ppo_loss_grad's gradients: w_ih [4H,17], w_hh [4H,H], b_ih [4H], b_hh [4H], the trunk's
 * layers (w [out,in] then b [out], the head last), log_std [6] last for an actor.  actor_grad [P,Ga], critic_grad [P,Gc]:
 * RdvLstmPpoSetOut's (a plain pair: RdvLstmPpoOut's).  Base pointers 16-byte aligned; rows are 4-byte aligned only and every access to
 * them is one float.  The arrays must not alias one another, and the parameter rows must hold the weights the blocks were packed from.
 *
 * The contract is that of rdv_ppo_set_adam_step, restated.  For every active member g (bit g of active_mask):
 *   - Norm.  ONE 2-norm over the member's Ga + Gc gradient entries.  The squares are added in double, in an order fixed by the index
 *     alone, with no floating-point atomic: the concatenation [actor row | critic row] is cut into chunks of 4096 entries (the last may
 *     be short); within chunk c thread t of 256 adds the squares of entries 4096 c + t, + 256, .. in index order, and the 256 sums are
 *     added by the halving tree (t += t + 128, then + 64, .. + 1); the chunk sums are then added in chunk order.  The square root is
 *     taken in double and rounded to float once.
 *   - clip_coef, step_size, inv_sqrt_bc2, coef[g] (8 floats) and step[g] <- step[g] + 1: exactly as stated under rdv_ppo_set_adam_step.
 *   - Elementwise: the same four float32 lines (g', m, v, p), every operation rounded on its own, `/` and sqrt correctly rounded.
 *   - Non-finite.  A member whose total_norm is not finite is skipped whole: its parameters, moments, step and both blocks are
 *     untouched, coef[g] = total_norm, 0, 0, 0, 1, 0, 0, 0; the other members are unaffected.
 *   - Repack.  After the step member g's two forward blocks [trunk block | cell block] are the bytes that rdv_lstm_policy_create /
 *     rdv_lstm_critic_create pack from its new fp32 parameters.  Trunk block: the fragments with layer 0 = [hidden[0], H] in natural k
 *     order over H / 16 k-steps and later layers in accumulator order, zero fragments and rows for 16- and 32-wide layers and for the
 *     head's rows >= out_dim, the biases in accumulator order times 2^(10 + s), each layer's inverse scale in its record, log_std.  Cell
 *     block: ONE shift for [W_ih | W_hh] — min(s_ih, s_hh), which is the shift of the larger of the two maxima since the rule is monotone
 *     — its inverse scale at float 0, the fragments [term][tile = q H / 32 + j][ks] (k-steps 0 and 1: the 17 inputs zero-padded, then the
 *     H / 16 k-steps of h), b_ih then b_hh, each [tile][lane half][16], times the accumulator's scale.  Only live floats are written:
 *     the header words, the H word of the cell header, the 64 zero floats and the records' integers are the host packer's and stay.
 *     Nothing is read back from a block: the fp32 master rows are the source.
 *     ONE EXCEPTION: the six exp(log_std) floats of an actor block.  The device writes the double-precision exp rounded to float; the host
 *     packer of the recurrent blocks writes the C library's exp on the float (unchanged by this call's introduction).  The device's float
 *     is within 1 ulp of the correctly rounded float(exp(log_std)), hence within 2 ulp of the host packer's.  What follows: after a device
 *     step "row i of member g equals a stand-alone handle of member g's weights" holds by equality for the deterministic action and the
 *     value, which do not read exp(log_std) (and for the state h, c, which no trunk float enters); SAMPLED actions, their log_prob and
 *     the rdv_lstm_ppo_* gradients read it from the block and equal those of a handle packed on the host from the same weights wherever
 *     the two floats are equal, and differ by the noise times at most 2 ulp of std otherwise.
 *   - An inactive member (mask bit clear): nothing of it is read or written — rows, blocks, coef[g], step[g], nor its slice of the workspace.
 *
 * The call:
 *   - The handles' LSTM state (h, c) and pending flags are neither read nor written.
 *   - Enqueue only: no allocation, no synchronisation, no host-device copy; legal inside a stream capture, and each replay of a captured
 *     graph takes the NEXT step.  Launches queued earlier on the stream read the old blocks, later ones the new blocks.  Deterministic:
 *     the same bits eager or replayed.  4 launches: chunk sums; coefficients; step and per-layer partial maxima; repack.
 *   - workspace: the caller's, 16-byte aligned, rdv_lstm_ppo_adam_workspace_bytes(specs, P) bytes: per member the chunk sums (doubles)
 *     and the partial maxima of |p| per (net, layer, chunk).  Its contents mean nothing between calls.
 *   - rdv_lstm_ppo_adam_workspace_bytes (host only): -1 for a bad pair of specs (rdv_lstm_ppo_spec_check: different hidden sizes
 *     included) or n_members outside 1..64; otherwise a multiple of 16, monotone in n_members.
 *   - Order of checks.  The host-only checks of rdv_ppo_set_adam_step with the same messages under this call's name (null state or
 *     pointer, misaligned array, lr, eps, the betas, max_grad_norm, an empty mask, a mask bit at or beyond the member count); a null, then
 *     a misaligned workspace; RDV_ERR_BAD_HANDLE for an invalid handle; then RDV_ERR_INVALID_ARGUMENT, in the order of
 *     rdv_lstm_ppo_set_loss_grad, for a handle that is not recurrent, swapped sets, different member counts, more than 64 members,
 *     different hidden sizes, different devices, a short workspace.  A refused call enqueues nothing.
 */
int64_t rdv_lstm_ppo_adam_workspace_bytes(const RdvLstmSpec* actor_spec_host, const RdvLstmSpec* critic_spec_host, int32_t n_members);
int rdv_lstm_ppo_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state,
                               const float* actor_grad, const float* critic_grad, uint64_t active_mask,
                               double lr, double beta1, double beta2, double eps, double max_grad_norm,
                               void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDV_H_ */

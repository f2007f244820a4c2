// rdv_hip.hip — the host side of the MI355X-native batched rendezvous environment: the C ABI of include/rdv.h for env handles
// (parameter groups, argument checks, launches, snapshot / restore, statistics) and rdv_rollout, the derivation of the thresholds the
// kernels compare against (derive_params), rigid-body validation and the workspace layout.  Its kernels are instantiated from the headers
// included below: rdv_step.h and rdv_fused.h (one-launch step kernels), rdv_cold.h (reset, state access, evaluation summary),
// rdv_policy.h (the shipped actor / critic, launched through shipped_launch_*), rdv_rollout.h and rdv_step_many.h (persistent kernels);
// three small ones (parameter upload, device error word, snapshot header) are defined here.  rdv_tiles.hip, rdv_general.hip,
// rdv_groups.hip (which instantiates the step kernels of rdv_step.h and rdv_fused.h once more, with a tile table), rdv_policy_mlp.hip,
// rdv_policy_lstm.hip, rdv_policy_sets.hip (the actor / critic kernels of policy sets) and rdv_advantages.hip are translation units of
// their own, entered through the launch functions of their headers; rdv_policy_host.hip is the host side of the policy handles and has
// no kernel (rdv_host.h: what it shares with this file).  The data layout in HBM is described in rdv_kernels.h.
#include "rdv_device.h"
#include "rdv_policy.h"
#include "rdv_host.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/rdv.h"

#include "rdv_kernels.h"
#include "rdv_fused.h"
#include "rdv_slots.h"
#include "rdv_step.h"
#include "rdv_cold.h"
#include "rdv_rollout.h"
#include "rdv_step_many.h"
#include "rdv_tiles.h"
#include "rdv_general.h"
#include "rdv_groups.h"
#include "rdv_launch.h"
#include "rdv_policy_sets.h"

namespace rdv {
static_assert(kGroupTile == kSetTile, "one rule (rdv_param_groups_check) and one table (rdv_host.h: tile_table) serve parameter groups and policy sets");

// ---------------------------------------------------------------------------------------------------------------
// host side
static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {   // (rdv_host.h: rdv_policy_host.hip reports through it too)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
static inline int64_t n_waves(int64_t n) { return (n + kBlock - 1) / kBlock * (kBlock / kWave); }
// Chunk stride (in envs): chunk c of env i is vector c * stride + i of the workspace.  The seven chunk arrays are walked in
// lockstep, and every BASELINE size puts them a power of two apart; padding each array to 64 KiB / 2 MiB and offsetting neighbours by
// 4 ... 260 KiB was measured (tools/chunk_skew_sweep.py, profiles/r02_chunk_skew.txt): 3-5 % at 0.5-1 M envs under the plain block
// order, nothing on top of the XCD-contiguous order (xcd_order_by_size), which gains more — so the arrays lie back to back.  RDV_CHUNK_ALIGN / RDV_CHUNK_SKEW (bytes, multiples of 256) in the environment set a padded spacing for that tool.
static inline int64_t chunk_stride(int64_t n, int storage) {
  static const int64_t align = [] { const char* x = getenv("RDV_CHUNK_ALIGN"); const long long v = x ? atoll(x) : 0; return (int64_t)(v >= 256 && v % 256 == 0 ? v : 0); }();
  static const int64_t skew = [] { const char* x = getenv("RDV_CHUNK_SKEW"); const long long v = x ? atoll(x) : 0; return (int64_t)(v >= 0 && v % 256 == 0 ? v : 0); }();
  if (align == 0) return n;
  const int64_t vb = 4 * (storage == RDV_STORAGE_F64 ? 8 : 4);
  return (align_up(n * vb, align) + skew) / vb;
}
constexpr int kAcosEntries = 200001;   // acos(k/1e5), k = -100000..100000 (general.py:179 rounds every cosine to 5 decimals)
// The workspace: ten regions back to back in this order, each padded to 256 bytes (byte offsets; snapshots and caller-provided
// workspaces depend on order, padding and sizes).
struct WorkspaceLayout {
  int64_t chunks, stats;    // the seven chunk arrays, the statistics slots: together the payload of a snapshot
  int64_t params, acos;     // device copy of DevParams, the acos table
  int64_t prep, prep_tag;   // prepared next-episode states (rdv_slots.h): one record per env (7 chunks + 5 float4 of observation), one tag per env
  int64_t eval_partial;     // per-wave partial sums of eval_summary_kernel
  int64_t dev_error;        // the handle's device error word (RdvDeviceError bits), alone in its line
  int64_t act_tmp, obs_tmp; // clipped actions of rdv_rollout's act + step form, and its observation rows when [t][N][17] rows are not 16-byte aligned
  int64_t total;
};
static WorkspaceLayout workspace_layout(int64_t n, int storage) {
  const bool f64 = storage == RDV_STORAGE_F64;
  WorkspaceLayout L;
  int64_t at = 0;
  auto region = [&](int64_t bytes) { const int64_t offset = at; at += align_up(bytes, 256); return offset; };
  L.chunks = region(kChunks * chunk_stride(n, storage) * 4 * (f64 ? 8 : 4));
  L.stats = region(n_waves(n) * kStatWords * (int64_t)sizeof(uint64_t));
  L.params = region((int64_t)sizeof(DevParams));
  L.acos = region((int64_t)kAcosEntries * (int64_t)sizeof(double));
  L.prep = region(n * (f64 ? slot_record_bytes<double>() : slot_record_bytes<float>()));
  L.prep_tag = region(n * 4);
  L.eval_partial = region(n_waves(n) * EV_SLOTS * (int64_t)sizeof(double));
  L.dev_error = region(sizeof(uint32_t));
  L.act_tmp = region(n * RDV_ACT_DIM * (int64_t)sizeof(float));
  L.obs_tmp = region(n * RDV_OBS_DIM * (int64_t)sizeof(float));
  L.total = at;
  return L;
}

// Largest integer k in [-100000, 100000] for which acos(k/1e5) > theta (strict) or >= theta; -100001 if there is none.
// acos(k/1e5) is what general.py:179 evaluates for every cosine that rounds to k*1e-5, so comparing k with this
// threshold is the reference's comparison, decided once on the host with the libm the oracle uses.
static double largest_k_with_angle_above(double theta, bool strict) {
  long lo = -100001, hi = 100001;   // predicate true at lo (virtual), false at hi (virtual); acos is decreasing in k
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    const double ang = std::acos((double)mid / 1e5);
    const bool above = strict ? (ang > theta) : (ang >= theta);
    if (above) lo = mid; else hi = mid;
  }
  return (double)lo;
}

static inline double norm3h(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// Largest double T >= 0 with sqrt(T) <= limit (strict: sqrt(T) < limit), -1 if there is none: T decides, for a sum of squares s,
// exactly what the reference's `np.linalg.norm(x) <= limit` decides for sqrt(s) (std::sqrt is correctly rounded, as NumPy's).
static double sq_threshold(double limit, bool strict) {
  auto ok = [&](double v) { const double r = std::sqrt(v); return strict ? r < limit : r <= limit; };
  if (limit != limit || !ok(0.0)) return -1.0;
  if (std::isinf(limit)) return strict ? 1.79769313486231570815e308 : limit;
  double x = limit * limit;
  if (std::isinf(x)) x = 1.79769313486231570815e308;
  while (x > 0.0 && !ok(x)) x = std::nextafter(x, 0.0);
  while (x < 1.79769313486231570815e308 && ok(std::nextafter(x, INFINITY))) x = std::nextafter(x, INFINITY);
  return x;
}

static void derive_params(const RdvParams& p, DevParams& d) {
  std::memset(&d, 0, sizeof d);
  const double n = p.n, t = p.dt, nt = n * t, c = std::cos(nt), s = std::sin(nt);
  // dynamics.py:40-47, expression for expression
  d.phi_xx = 4 - 3 * c;          d.phi_xvx = 1 / n * s;         d.phi_xvy = 2 / n * (1 - c);
  d.phi_yx = 6 * (s - nt);       d.phi_yvx = -2 / n * (1 - c);  d.phi_yvy = 1 / n * (4 * s - 3 * nt);
  d.phi_zz = c;                  d.phi_zvz = 1 / n * s;
  d.phi_vxx = 3 * n * s;         d.phi_vxvx = c;                d.phi_vxvy = 2 * s;
  d.phi_vyx = -6 * n * (1 - c);  d.phi_vyvx = -2 * s;           d.phi_vyvy = 4 * c - 3;
  d.phi_vzz = -n * s;            d.phi_vzvz = c;
  d.dt = p.dt; d.half_dt = 0.5 * p.dt;
  d.max_delta_w = p.max_delta_w;
  d.max_delta_v_f32 = (float)p.max_delta_v;
  d.fuel_scale_f32 = (float)(p.dt * p.fuel_coef);
  d.fuel_div_f32 = (float)(3 * p.max_delta_v);
  {  // :193 t = round(t + dt, 3), :368 t >= t_max  ->  first step count whose rounded time reaches t_max (dt is a multiple of 1 ms:
     // rdv_params_validate; then the running sum IS rint(k*dt*1e3)/1e3, tests/golden/thresholds_reference.npz)
    long long k = (long long)std::floor(p.t_max / p.dt) - 3;
    if (k < 0) k = 0;
    while (k < 2147483647LL && std::rint((double)k * p.dt * 1e3) / 1e3 < p.t_max) ++k;
    d.k_time = (int32_t)k;
  }
  d.obs_lo_r = -p.max_axial_distance; d.obs_span_r = p.max_axial_distance - (-p.max_axial_distance); d.obs_inv_span_r = 1.0 / d.obs_span_r;
  d.obs_lo_v = -p.max_axial_speed;    d.obs_span_v = p.max_axial_speed - (-p.max_axial_speed);       d.obs_inv_span_v = 1.0 / d.obs_span_v;
  d.obs_lo_w = -p.max_wc;             d.obs_span_w = p.max_wc - (-p.max_wc);                         d.obs_inv_span_w = 1.0 / d.obs_span_w;
  d.koz_radius = p.koz_radius; d.corridor_half_angle = p.corridor_half_angle;
  d.inv_max_attitude_error = 1.0 / p.max_attitude_error; d.inv_max_rd_error = 1.0 / p.max_rd_error; d.inv_max_qd_error = 1.0 / p.max_qd_error;
  for (int i = 0; i < 3; ++i) { d.corridor_axis[i] = p.corridor_axis[i]; d.capture_axis[i] = p.capture_axis[i]; d.rd[i] = p.rd[i]; }
  d.inv_corridor_norm = 1.0 / norm3h(p.corridor_axis); d.inv_capture_norm = 1.0 / norm3h(p.capture_axis);
  d.le2_rd = sq_threshold(p.max_rd_error, false); d.lt2_rd = sq_threshold(p.max_rd_error, true);        // :416 (<=), :348 (<)
  d.le2_vd = sq_threshold(p.max_vd_error, false); d.le2_wd = sq_threshold(p.max_wd_error, false);       // :416-417
  d.lt2_vd = sq_threshold(p.max_vd_error, true); d.lt2_wd = sq_threshold(p.max_wd_error, true);         // monte_carlo.py:160, :162 (<)
  d.lt2_koz = sq_threshold(p.koz_radius, true);                                                        // :397, :340
  {  // an initial state can only be inside the KOZ sphere or meet the capture position error within this radius of the target
    const double rr = std::fmax(p.koz_radius, norm3h(p.rd) + p.max_rd_error) * (1.0 + 1e-9);
    d.reset_flag_radius2 = rr * rr;
  }
  d.kc_coll_max = largest_k_with_angle_above(p.corridor_half_angle, true);        // :401  angle >  half_angle
  d.ka_done_max = largest_k_with_angle_above(p.max_attitude_error, true);         // :370  att   >  max_attitude_error
  d.ka_succ_min = largest_k_with_angle_above(p.max_qd_error, true) + 1.0;         // :417  att   <= max_qd_error
  d.ka_bonus_min = largest_k_with_angle_above(p.max_qd_error, false) + 1.0;       // :350  att   <  max_qd_error
  d.bubble_radius0 = p.bubble_radius0; d.bubble_decrease_rate = p.bubble_decrease_rate; d.bubble_min = p.bubble_min;
  d.att_term = p.dt * p.att_coef; d.coll_term = p.dt * p.collision_coef; d.bonus_term = p.dt * p.bonus_coef;
  for (int i = 0; i < 3; ++i) { d.nominal_rc0[i] = p.nominal_rc0[i]; d.nominal_vc0[i] = p.nominal_vc0[i]; d.nominal_wc0[i] = p.nominal_wc0[i]; d.nominal_wt0[i] = p.nominal_wt0[i]; }
  {  // quat_product normalises its factors (quaternions.py:159-160)
    const double mc = std::sqrt(p.nominal_qc0[0] * p.nominal_qc0[0] + p.nominal_qc0[1] * p.nominal_qc0[1] + p.nominal_qc0[2] * p.nominal_qc0[2] + p.nominal_qc0[3] * p.nominal_qc0[3]);
    const double mt = std::sqrt(p.nominal_qt0[0] * p.nominal_qt0[0] + p.nominal_qt0[1] * p.nominal_qt0[1] + p.nominal_qt0[2] * p.nominal_qt0[2] + p.nominal_qt0[3] * p.nominal_qt0[3]);
    for (int i = 0; i < 4; ++i) { d.nominal_qc0[i] = p.nominal_qc0[i] / mc; d.nominal_qt0[i] = p.nominal_qt0[i] / mt; }
  }
  d.rc0_range = p.rc0_range; d.vc0_range = p.vc0_range; d.qc0_range = p.qc0_range;
  d.wc0_range = p.wc0_range; d.qt0_range = p.qt0_range; d.wt0_range = p.wt0_range;
  d.qc0_tiny = (0.25 * p.qc0_range * p.qc0_range <= kTinyU) ? 1 : 0;   // theta = range * u, 0 < u < 1 (deviate)
  d.qt0_tiny = (0.25 * p.qt0_range * p.qt0_range <= kTinyU) ? 1 : 0;
}

// The derived parameter block travels as a kernel argument and is written by the device: ordered on the caller's stream like
// every other launch (a hipMemcpy from host memory is ordered against the legacy stream only, not against PyTorch's non-blocking
// side streams) and legal inside a stream capture (the values are baked into the graph node).
__global__ __launch_bounds__(kWave) void params_kernel(const DevParams src, DevParams* dst) {
  const uint32_t* from = reinterpret_cast<const uint32_t*>(&src);
  uint32_t* to = reinterpret_cast<uint32_t*>(dst);
  for (int k = threadIdx.x; k < (int)(sizeof(DevParams) / 4); k += kWave) to[k] = from[k];
}
// rdv_debug_set_device_error: what a kernel that detects a fault does to the handle's error word
__global__ __launch_bounds__(kWave) void device_error_kernel(uint32_t* word, uint32_t bits) {
  if (threadIdx.x == 0) __hip_atomic_fetch_or(word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static_assert(sizeof(DevParams) % 4 == 0 && sizeof(DevParams) <= 3072, "DevParams is passed by value to params_kernel");

}  // namespace rdv

using namespace rdv;

struct RdvEnvBatch {
  uint32_t magic;
  RdvParams params;
  DevParams dev;
  int64_t n;
  int device, storage, on_done;
  uint64_t seed, env_id_offset;
  void* ws;          // chunks
  uint64_t* stats;   // slots
  DevParams* dev_params;   // device copy of `dev`, read by the step kernels
  double* acos_table;      // device, kAcosEntries doubles
  bool own_ws;
  bool fresh;        // no reset yet since create/seed
  const double* tape;
  int32_t tape_depth;
  int variant;       // RdvKernelVariant
  int64_t cs;        // chunk stride in envs (chunk_stride)
  int xcd_order;     // fused kernels' block order: -1 by size (xcd_order_by_size), 0 plain, 1 XCD-contiguous
  int split_general; // general target: step_kernel_general (1, default) or the fused per-lane kernel for both bodies (RDV_GENERAL_SPLIT=0, diagnostics)
  int tiles_grid;    // RDV_VARIANT_FUSED_TILES: grid in workgroups (0: kTilesPerCU per CU; RDV_TILES_GRID in the environment, diagnostics)
  int n_cus;         // compute units of the device
  RdvRigidBody body; // rdv_set_rigid_body
  bool general;      // step with the RK45 kernels (body is not isotropic / torque-free, or RK45 was asked for)
  bool raw_state;    // rdv_set_state since the last step: quaternions may be unnormalised (next step: kRaw kernel)
  const char* last_kernel;  // name of the step kernel the last rdv_step / rdv_step_many / rdv_rollout launched (rdv_debug_last_kernel)
  void* prep;        // prepared next-episode states (rdv_slots.h): records, tags
  uint32_t* prep_tag;
  double* eval_partial;   // per-wave partial sums of rdv_eval_summary
  uint32_t* dev_error;    // device error word (RdvDeviceError bits), set by kernels with an atomic OR
  float* act_tmp;         // [N,6] clipped actions between rdv_policy_act and rdv_step inside rdv_rollout's act + step form
  float* obs_tmp;         // [N,17] aligned observation rows of the act + step forms when N is not a multiple of 4
  uint32_t device_error;  // host copy: what the synchronising calls have read so far (sticky)
  uint32_t host_error_word;
  std::vector<double> host_eval;
  bool prepared_ok;  // every slot holds what the env's next reset returns (false: prepare_kernel runs before the next slot-using launch)
  // step_kernel_split's slot form asks less of the slots and keeps them so itself: a tag that equals episode + 1 tells the truth (rdv_step.h).
  // False after whatever clears prepared_ok from outside and after every rdv_step launch of another kernel (they advance episodes in
  // registers); prepare_kernel then runs in front of the next slot-form launch.
  bool step_slots_ok;
  int split_form;    // step_kernel_split, fp32 storage, RESET: 3 the target form with the observation on the service waves too, 2 the slot form with the target's side on the service waves, 1 the slot form, 0 the speculative reset (RDV_SPLIT_FORM=slots_target_obs|slots_target|slots|speculative in the environment of rdv_create; default: split_slots_by_size, split_target_by_size, split_obs_by_size)
#ifdef RDV_STAMPS
  unsigned long long* stamps = nullptr;
#endif
  std::vector<uint64_t> host_slots;
  // parameter groups (rdv_set_param_groups): n_groups == 0 is the single block above.  The G blocks and the tile table are a side
  // allocation of their own (the workspace layout, which snapshots and caller-provided workspaces depend on, does not change).
  int32_t n_groups = 0;
  std::vector<RdvParams> group_params;
  std::vector<DevParams> group_dev;
  std::vector<int64_t> group_start;      // [G + 1]: group g is envs [group_start[g], group_start[g + 1])
  void* group_mem = nullptr;             // device: G blocks, then the tile table
  size_t group_mem_bytes = 0;
  GroupTable group_table = {nullptr, nullptr};
};
static constexpr uint32_t kMagic = 0x52445631u;   // "RDV1"
static void derive_block(const RdvEnvBatch* h, const RdvParams& p, DevParams& dev);

#define RDV_CHECK_HANDLE(h) \
  if (!(h) || (h)->magic != kMagic) return fail(RDV_ERR_BAD_HANDLE, "invalid rdv_handle")
// calls that launch work on a handle refuse once a device fault has been read back (sticky: the state may be corrupt)
#define RDV_CHECK_FAULT(h) \
  if ((h)->device_error) return rdv_device_error_code((h)->device_error)

// the fields StepArgs, StepManyArgs and RolloutArgs share by name, from the handle (the callers add their I/O pointers)
template <class Args>
static void fill_batch_fields(Args& A, const RdvEnvBatch* h) {
  A.ws = h->ws; A.stats = h->stats; A.tape = h->tape; A.n = h->n; A.cs = h->cs; A.seed = h->seed; A.env_id_offset = h->env_id_offset;
  A.tape_depth = h->tape_depth; A.on_done = h->on_done; A.prep = h->prep; A.prep_tag = h->prep_tag;
}
static void base_args(const RdvEnvBatch* h, StepArgs& A) {
  std::memset(&A, 0, sizeof A);
  fill_batch_fields(A, h);
}
static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
static inline dim3 policy_grid(int64_t n) { return dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)); }
// f(ST()) with ST the storage type of a batch: the env kernels are templates over it.  (The deduced return type has the call
// instantiated where it stands, so the kernels are emitted in the order of the launch sites in this file.)
template <class F>
static inline auto with_storage(int storage, F&& f) {
  if (storage == RDV_STORAGE_F32) return f(float());
  return f(double());
}
// The handle's device error word, read back on `s` behind whatever the caller has enqueued there: this synchronises the stream and
// leaves the bits in h->device_error (sticky).  `clear_stats_bytes`: rdv_get_stats zeroes that much of the statistics between the copy
// and the wait.
static int read_fault_word(RdvEnvBatch* h, hipStream_t s, size_t clear_stats_bytes = 0) {
  RDV_HIP(hipMemcpyAsync(&h->host_error_word, h->dev_error, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (clear_stats_bytes) RDV_HIP(hipMemsetAsync(h->stats, 0, clear_stats_bytes, s));
  RDV_HIP(hipStreamSynchronize(s));
  h->device_error |= h->host_error_word;
  return RDV_OK;
}

// The persistent kernels (step_many_kernel, rollout_kernel) rely on every slot holding what the env's next reset returns.
// Whatever changes that from outside them (parameters, tape, seed, restore) or advances episodes without them (rdv_step) clears
// prepared_ok; the slots are then re-derived here, on the caller's stream, before the next such launch.
static int ensure_prepared(RdvEnvBatch* h, hipStream_t s) {
  if (h->on_done != RDV_ON_DONE_RESET || h->prepared_ok) return RDV_OK;
  StepArgs A;
  base_args(h, A);
  with_storage(h->storage, [&](auto st) { hipLaunchKernelGGL(prepare_kernel<decltype(st)>, grid_for(h->n), dim3(kBlock), 0, s, h->dev_params, A); });
  RDV_HIP(hipGetLastError());
  h->prepared_ok = true;
  h->step_slots_ok = true;
  return RDV_OK;
}
// ... and the slot form of step_kernel_split on the slots' tags telling the truth (step_slots_ok).  prepare_kernel is idempotent, so a
// capture that begins with the flag down simply records it in front of its first step.
static int ensure_step_slots(RdvEnvBatch* h, hipStream_t s) {
  if (h->step_slots_ok) return RDV_OK;
  const bool was = h->prepared_ok;
  h->prepared_ok = false;
  const int rc = ensure_prepared(h, s);
  if (rc) h->prepared_ok = was;
  return rc;
}
// The loops of rdv_step that rdv_step_many and rdv_rollout are defined by write row t of the caller's [T][N][17] observations from a kernel
// that stores 16-byte vectors: the row is aligned if and only if N % 4 == 0.  Otherwise the kernel writes h->obs_tmp and the row is a copy.
static inline bool obs_rows_aligned(const RdvEnvBatch* h) { return (h->n & 3) == 0; }
static inline float* obs_row_target(const RdvEnvBatch* h, float* obs, int64_t t) { return obs_rows_aligned(h) ? obs + t * h->n * RDV_OBS_DIM : h->obs_tmp; }
static int obs_row_flush(const RdvEnvBatch* h, float* obs, int64_t t, hipStream_t s) {
  if (!obs_rows_aligned(h)) RDV_HIP(hipMemcpyAsync(obs + t * h->n * RDV_OBS_DIM, h->obs_tmp, (size_t)h->n * RDV_OBS_DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
  return RDV_OK;
}
// the derived parameter block -> device, ordered on `s` (params_kernel)
static int upload_params(RdvEnvBatch* h, hipStream_t s) {
  hipLaunchKernelGGL(params_kernel, dim3(1), dim3(kWave), 0, s, h->dev, h->dev_params);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// The shipped actor / critic (rdv_policy.h: policy_act_kernel, policy_value_kernel) for rdv_policy_host.hip, in the shape of
// rdv_policy_mlp.h's trio; the limit is raised when a handle that will run them is created.
hipError_t rdv::shipped_raise_lds_limit() {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_act_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPolLdsBytes);
  if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_value_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPolLdsBytes);
  return err;
}
void rdv::shipped_launch_act(int, const float* W, int, const float* obs, float* actions, int64_t n, int deterministic, uint64_t seed, uint64_t counter,
                             uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  hipLaunchKernelGGL(policy_act_kernel, policy_grid(n), dim3(kPolBlock), kPolLdsBytes, s, W, obs, actions, n, deterministic, seed,
                     counter, env_id_offset, raw_actions, log_prob);
}
void rdv::shipped_launch_value(int, const float* W, int, const float* obs, float* values, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(policy_value_kernel, policy_grid(n), dim3(kPolBlock), kPolLdsBytes, s, W, obs, values, n);
}

extern "C" {

int rdv_version(void) { return RDV_ABI_VERSION; }
const char* rdv_last_error(void) { return g_err; }

int rdv_device_error_code(uint32_t word) {
  if (word == 0u) return RDV_OK;
  char what[256] = "";
  if (word & RDV_DEVERR_LOST_SIGNAL) std::strncat(what, " LOST_SIGNAL (rdv_rollout: an env wave's bounded wait for its workgroup's slot-refill signal expired)", sizeof what - std::strlen(what) - 1);
  if (word & ~(uint32_t)RDV_DEVERR_LOST_SIGNAL) std::strncat(what, " unknown bits", sizeof what - std::strlen(what) - 1);
  return fail(RDV_ERR_DEVICE_FAULT, "device error word 0x%x:%s; results of this handle since the fault are not to be trusted", word, what);
}

int rdv_debug_set_device_error(rdv_handle h, uint32_t bits, void* stream) {
  RDV_CHECK_HANDLE(h);
  DeviceGuard guard(h->device);
  hipLaunchKernelGGL(device_error_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), h->dev_error, bits);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

const char* rdv_debug_last_kernel(rdv_handle h) {
  if (!h || h->magic != kMagic) { fail(RDV_ERR_BAD_HANDLE, "invalid rdv_handle"); return nullptr; }
  return h->last_kernel;
}

int rdv_params_default(RdvParams* p) {
  if (!p) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_params_default: null output");
  std::memset(p, 0, sizeof *p);
  const double rad = 3.14159265358979323846 / 180.0;
  p->nominal_rc0[1] = -10.0; p->nominal_qc0[0] = 1.0; p->nominal_qt0[0] = 1.0;          // rendezvous_env.py:52-57
  p->rc0_range = 1.0; p->vc0_range = 0.1; p->qc0_range = 1.0 * rad; p->wc0_range = 0.1 * rad;
  p->qt0_range = 45.0 * rad; p->wt0_range = 3.0 * rad;                                   // :60-65
  p->dt = 1.0; p->t_max = 120.0;                                                        // :69-70
  const double mass = 100.0, inertia = 1.0 * 1.0 / 12.0 * mass * 2.0;                    // :74-79
  p->max_delta_v = 10.0 / mass * 0.5; p->max_delta_w = 0.2 / inertia * 0.5;              // :81-82
  p->max_axial_distance = 10.0 + 10.0; p->max_axial_speed = 5.0; p->max_wc = 10.0 * rad; // :85-87
  p->max_attitude_error = 30.0 * rad;                                                    // :89
  p->koz_radius = 5.0; p->corridor_half_angle = 30.0 * rad;                              // :93-94
  p->corridor_axis[1] = -1.0; p->capture_axis[1] = 1.0; p->rd[1] = -2.0;                 // :95, :73, :104
  p->max_rd_error = 0.5; p->max_vd_error = 0.1; p->max_qd_error = 5.0 * rad; p->max_wd_error = 1.0 * rad;   // :105-108
  p->bubble_radius0 = p->max_axial_distance; p->bubble_decrease_rate = 0.5 * p->dt;      // :114-115
  p->bubble_min = 2.0 + 2.0 * p->max_rd_error;                                           // :116
  const double mu = 3.986004418e14, ro = 6371e3 + 800e3;                                 // :122-125
  p->n = std::sqrt(mu / (ro * ro * ro));                                                 // :126
  p->collision_coef = 0.5; p->bonus_coef = 8.0; p->fuel_coef = 0.2; p->att_coef = 1.0;   // :313
  return RDV_OK;
}

int rdv_params_validate(const RdvParams* p) {
  if (!p) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_params_validate: null params");
  const double* d = reinterpret_cast<const double*>(p);
  for (size_t i = 0; i < sizeof(RdvParams) / sizeof(double); ++i)
    if (!std::isfinite(d[i])) return fail(RDV_ERR_BAD_PARAMS, "parameter #%zu is not finite", i);
  const double rdn = std::sqrt(p->rd[0] * p->rd[0] + p->rd[1] * p->rd[1] + p->rd[2] * p->rd[2]);
  if (!(rdn < p->koz_radius)) return fail(RDV_ERR_BAD_PARAMS, "Error: terminal position lies outside corridor.");        // :155
  if (!(rdn - p->max_rd_error > 0)) return fail(RDV_ERR_BAD_PARAMS, "Error: position constraint allows collisions");   // :156
  if (!(p->dt > 0) || !(p->n > 0) || !(p->max_axial_distance > 0) || !(p->max_axial_speed > 0) || !(p->max_wc > 0) ||
      !(p->max_attitude_error > 0) || !(p->max_rd_error > 0) || !(p->max_qd_error > 0) || !(p->max_delta_v > 0))
    return fail(RDV_ERR_BAD_PARAMS, "dt, n, the observation scales and the error limits must be positive");
  // :193 t = round(t + dt, 3).  For dt = j/1000 (as a double) every running sum rounds to the decimal k*j/1000, which is what k_time and
  // the reported t assume (derive_params); for any other dt the reference's sum drifts away from round(k*dt, 3) — 1/3 s reaches
  // t_max = 60 on step 181, 0.0125 s reaches 5 on step 398 — so such a dt is refused, not stepped on another clock than the reference's.
  if (!(p->dt == std::rint(p->dt * 1e3) / 1e3))
    return fail(RDV_ERR_BAD_PARAMS, "dt = %.17g s is not a multiple of 0.001 s: the reference's round(t + dt, 3) drifts for such a dt "
                                    "(its running sum leaves round(k*dt, 3)), so episode times and the time limit would differ", p->dt);
  return RDV_OK;
}

int64_t rdv_workspace_bytes(int64_t n_envs, int storage) {
  if (n_envs <= 0 || (storage != RDV_STORAGE_F32 && storage != RDV_STORAGE_F64)) return -1;
  return workspace_layout(n_envs, storage).total;
}

int64_t rdv_num_envs(rdv_handle h) { return (h && h->magic == kMagic) ? h->n : -1; }

int rdv_rollout(rdv_handle h, rdv_policy p, int32_t n_steps, const RdvRolloutOut* out, int deterministic, uint64_t noise_seed,
                uint64_t noise_counter0, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_POLICY(p);
  if (p->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: this handle is a critic (rdv_critic_create)");
  if (p->device != h->device) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: the policy lives on device %d, the envs on device %d", p->device, h->device);
  if (n_steps <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: n_steps must be positive (got %d)", n_steps);
  if (p->rows && p->rows != h->n) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: the policy (a set, or a recurrent policy) owns %lld rows, the batch has %lld envs", (long long)p->rows, (long long)h->n);
  if (!out || !out->obs || !out->actions || !out->reward || !out->done || !out->last_obs)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: obs, actions, reward, done and last_obs are required");
  if (misaligned(out->obs, 16) || misaligned(out->actions, 16) || misaligned(out->last_obs, 16))
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: obs, actions and last_obs must be 16-byte aligned");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout: call rdv_reset first (state is undefined until reset(), as in the reference)");
  RDV_CHECK_FAULT(h);
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->general || h->n_groups || !p->shipped_arch || p->n_members > 1 || p->lstm_hidden) {
    // General rigid bodies, parameter groups (no grouped persistent kernel), policy sets of more than one member (no persistent kernel for
    // sets), recurrent policies and policies of another architecture than the shipped one (the persistent kernel's registers and LDS are
    // laid out for 17-64-64-6 tanh): rdv_policy_act (rdv_lstm_act for a recurrent actor) + rdv_step, n_steps times, on `stream` — the
    // definition of this call's results, used as its implementation.  The per-lane RK45 inside the 168-register budget of the persistent
    // kernel's 12-wave workgroup spilled 120 dwords per lane and ran SLOWER than this loop (72 against 58 us per step at 65,536 envs,
    // round 2): not offered any more.
    const int64_t n = h->n;
    float* obs_t = obs_row_target(h, out->obs, 0);
    if (int rc = rdv_observe(h, obs_t, stream)) return rc;
    for (int32_t t = 0; t < n_steps; ++t) {
      if (int rc = obs_row_flush(h, out->obs, t, s)) return rc;
      if (int rc = policy_act_step(p, t, obs_t, out->done, h->act_tmp, n, deterministic ? 1 : 0, noise_seed, noise_counter0 + (uint64_t)t, h->env_id_offset,
                                   out->actions + (int64_t)t * n * RDV_ACT_DIM, out->log_prob ? out->log_prob + (int64_t)t * n : nullptr, s)) return rc;
      RdvStepOut so;
      std::memset(&so, 0, sizeof so);
      float* obs_next = (t + 1 < n_steps) ? obs_row_target(h, out->obs, t + 1) : out->last_obs;
      so.obs = obs_next; so.reward = out->reward + (int64_t)t * n; so.done = out->done + (int64_t)t * n;
      if (int rc = rdv_step(h, h->act_tmp, &so, stream)) return rc;
      obs_t = obs_next;
    }
    // a recurrent actor's state has moved past the last step: what was done there is the start its next call finds pending
    if (p->lstm_hidden) RDV_HIP(hipMemcpyAsync(p->lstm_pending, out->done + (int64_t)(n_steps - 1) * n, (size_t)n, hipMemcpyDeviceToDevice, s));
    return RDV_OK;
  }
  h->raw_state = false;   // the rollout kernel integrates injected (unnormalised) quaternions itself
  if (int rc = ensure_prepared(h, s)) return rc;
  RolloutArgs A;
  fill_batch_fields(A, h);
  A.obs = out->obs; A.actions = out->actions; A.reward = out->reward; A.done = out->done;
  A.log_prob = out->log_prob; A.last_obs = out->last_obs; A.dev_error = h->dev_error;
  A.noise_seed = noise_seed; A.noise_counter0 = noise_counter0; A.n_steps = n_steps; A.deterministic = deterministic ? 1 : 0;
#ifdef RDV_STAMPS
  A.stamps = h->stamps;
#endif
  const dim3 grid((unsigned)((h->n + kRollEnvs - 1) / kRollEnvs)), block(kRollBlock);
  with_storage(h->storage, [&](auto st) {
    using ST = decltype(st);
    hipLaunchKernelGGL((rollout_kernel<ST, false>), grid, block, roll_lds_bytes<ST>(), s, h->dev_params, p->weights, A);
  });
  h->last_kernel = h->storage == RDV_STORAGE_F32 ? "rollout_kernel<float, false>" : "rollout_kernel<double, false>";
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

int rdv_create(const RdvParams* params, int64_t n_envs, int device, int storage, int on_done, uint64_t seed,
               uint64_t env_id_offset, void* workspace, rdv_handle* out) {
  if (!params || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_create: null params/out");
  if (n_envs <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_create: n_envs must be positive (got %lld)", (long long)n_envs);
  if (storage != RDV_STORAGE_F32 && storage != RDV_STORAGE_F64) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_create: bad storage %d", storage);
  if (on_done != RDV_ON_DONE_RESET && on_done != RDV_ON_DONE_HALT && on_done != RDV_ON_DONE_CONTINUE) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_create: bad on_done %d", on_done);
  if (int rc = rdv_params_validate(params)) return rc;
  if (int rc = check_device("rdv_create", device)) return rc;
  if (workspace && misaligned(workspace, 256)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_create: workspace must be 256-byte aligned");
  DeviceGuard guard(device);
  RdvEnvBatch* h = new (std::nothrow) RdvEnvBatch();
  if (!h) return fail(RDV_ERR_OUT_OF_MEMORY, "rdv_create: host allocation failed");
  h->magic = kMagic; h->params = *params;
  (void)rdv_rigid_body_default(&h->body); h->general = false;
  h->raw_state = false;
  h->last_kernel = "";

  h->n = n_envs; h->cs = chunk_stride(n_envs, storage); h->device = device; h->storage = storage; h->on_done = on_done; h->seed = seed; h->env_id_offset = env_id_offset;
  h->tape = nullptr; h->tape_depth = 0; h->fresh = true; h->variant = RDV_VARIANT_AUTO;
  { const char* x = getenv("RDV_XCD_ORDER"); h->xcd_order = (x && (x[0] == '0' || x[0] == '1') && !x[1]) ? x[0] - '0' : -1; }
  { const char* x = getenv("RDV_GENERAL_SPLIT"); h->split_general = (x && x[0] == '0' && !x[1]) ? 0 : 1; }
  { const char* x = getenv("RDV_TILES_GRID"); const long v = x ? atol(x) : 0; h->tiles_grid = v > 0 && v <= 65536 ? (int)(v + 7) / 8 * 8 : 0; }
  { int cus = 0; h->n_cus = (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ? cus : 256; }
  const WorkspaceLayout L = workspace_layout(n_envs, storage);
  const int64_t bytes = L.total;
  if (workspace) { h->ws = workspace; h->own_ws = false; }
  else {
    hipError_t err = hipMalloc(&h->ws, (size_t)bytes);
    if (err != hipSuccess) { (void)hipGetLastError(); delete h; return fail(RDV_ERR_OUT_OF_MEMORY, "rdv_create: hipMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(err)); }
    h->own_ws = true;
  }
  char* const base = static_cast<char*>(h->ws);   // (L.chunks == 0)
  h->stats = reinterpret_cast<uint64_t*>(base + L.stats);
  h->dev_params = reinterpret_cast<DevParams*>(base + L.params);
  h->acos_table = reinterpret_cast<double*>(base + L.acos);
  h->prep = base + L.prep;
  h->prep_tag = reinterpret_cast<uint32_t*>(base + L.prep_tag);
  h->eval_partial = reinterpret_cast<double*>(base + L.eval_partial);
  h->dev_error = reinterpret_cast<uint32_t*>(base + L.dev_error);   // zeroed with the workspace
  h->device_error = 0u; h->host_error_word = 0u;
  h->act_tmp = reinterpret_cast<float*>(base + L.act_tmp);
  h->obs_tmp = reinterpret_cast<float*>(base + L.obs_tmp);
  h->prepared_ok = false; h->step_slots_ok = false;
  { const char* x = getenv("RDV_SPLIT_FORM"); h->split_form = (x && !strcmp(x, "slots_target_obs")) ? 3 : (x && !strcmp(x, "slots_target")) ? 2 : (x && !strcmp(x, "slots")) ? 1 : (x && !strcmp(x, "speculative")) ? 0 : -1; }
  derive_block(h, *params, h->dev);
  // every step of the set-up reports itself: which call failed, and why
  const char* what = "hipMemset of the workspace";
  hipError_t err = hipMemset(h->ws, 0, (size_t)bytes);
  if (err == hipSuccess) {
    what = "hipMemcpy of the acos table";
    std::vector<double> table((size_t)kAcosEntries);
    for (int k = 0; k < kAcosEntries; ++k) table[(size_t)k] = std::acos((double)(k - 100000) / 1e5);   // the oracle's expression (rdv_probe.hip: rdvprobe_fill_acos_table is its twin, for the tests: keep them in step)
    err = hipMemcpy(h->acos_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice);
  }
  if (err == hipSuccess) { what = "hipMemcpy of the parameter block"; err = hipMemcpy(h->dev_params, &h->dev, sizeof(DevParams), hipMemcpyHostToDevice); }
  // the persistent kernels use more dynamic LDS than the 64 KiB default limit; raised here, outside any stream capture
  auto raise_lds = [&](const void* fn, int bytes, const char* name) {
    if (err == hipSuccess) { what = name; err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
  };
  for (int st_id : {RDV_STORAGE_F32, RDV_STORAGE_F64})
    with_storage(st_id, [&](auto st) {
      using ST = decltype(st);
      const bool f32 = sizeof(ST) == 4;
      raise_lds(reinterpret_cast<const void*>(rollout_kernel<ST, false>), roll_lds_bytes<ST>(),
                f32 ? "hipFuncSetAttribute(rollout_kernel<float>, MaxDynamicSharedMemorySize)" : "hipFuncSetAttribute(rollout_kernel<double>, MaxDynamicSharedMemorySize)");
      raise_lds(reinterpret_cast<const void*>(step_many_kernel<ST, false>), many_lds_bytes<ST>(),
                f32 ? "hipFuncSetAttribute(step_many_kernel<float>, MaxDynamicSharedMemorySize)" : "hipFuncSetAttribute(step_many_kernel<double>, MaxDynamicSharedMemorySize)");
    });
  if (err != hipSuccess) {
    (void)hipGetLastError();
    if (h->own_ws) (void)hipFree(h->ws);
    delete h;
    return fail(err == hipErrorOutOfMemory ? RDV_ERR_OUT_OF_MEMORY : RDV_ERR_HIP, "rdv_create: %s failed: %s", what, hipGetErrorString(err));
  }
  h->host_slots.resize((size_t)(n_waves(n_envs) * kStatWords));
  *out = h;
  return RDV_OK;
}

int rdv_destroy(rdv_handle h) {
  RDV_CHECK_HANDLE(h);
  DeviceGuard guard(h->device);
  (void)hipDeviceSynchronize();
  if (h->own_ws) (void)hipFree(h->ws);
  if (h->group_mem) (void)hipFree(h->group_mem);
  h->magic = 0;
  delete h;
  return RDV_OK;
}

// ---- rigid bodies (SURVEY f-4) -------------------------------------------------------------------------------------
int rdv_rigid_body_default(RdvRigidBody* b) {
  if (!b) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rigid_body_default: null output");
  std::memset(b, 0, sizeof *b);
  const double mass = 100.0, inertia = 1.0 * 1.0 / 12.0 * mass * 2.0;   // :74-79, :96-100
  for (int i = 0; i < 3; ++i) { b->inertia_chaser[4 * i] = inertia; b->inertia_target[4 * i] = inertia; }
  b->rtol = 1e-7; b->atol = 1e-6;                                        // :567-568
  b->integrator = RDV_INTEGRATOR_AUTO;
  return RDV_OK;
}
static bool invert3(const double* m, double* inv) {   // adjugate / determinant (np.linalg.inv at :80, :101 uses LU: same to rounding)
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  inv[0] = c00 / det; inv[1] = (m[2] * m[7] - m[1] * m[8]) / det; inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  inv[3] = c01 / det; inv[4] = (m[0] * m[8] - m[2] * m[6]) / det; inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  inv[6] = c02 / det; inv[7] = (m[1] * m[6] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
  return true;
}
static bool closed_form_applies(const double* inertia, const double* torque) {   // c * Identity, zero torque: w x (I w) = 0
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      if (i != j ? inertia[3 * i + j] != 0.0 : inertia[3 * i + j] != inertia[0]) return false;
  return torque[0] == 0.0 && torque[1] == 0.0 && torque[2] == 0.0;
}
static int validate_rigid_body(const RdvRigidBody* b, bool* general) {
  if (!b) return fail(RDV_ERR_INVALID_ARGUMENT, "null RdvRigidBody");
  if (b->integrator != RDV_INTEGRATOR_AUTO && b->integrator != RDV_INTEGRATOR_EXACT && b->integrator != RDV_INTEGRATOR_RK45)
    return fail(RDV_ERR_INVALID_ARGUMENT, "RdvRigidBody: bad integrator %d", b->integrator);
  const double* tensors[2] = {b->inertia_chaser, b->inertia_target};
  const char* names[2] = {"inertia_chaser", "inertia_target"};
  for (int k = 0; k < 2; ++k) {
    const double* m = tensors[k];
    for (int i = 0; i < 9; ++i) if (!std::isfinite(m[i])) return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: %s is not finite", names[k]);
    // a physical inertia tensor is symmetric positive definite (Sylvester's criterion)
    const double tol = 1e-12 * (std::fabs(m[0]) + std::fabs(m[4]) + std::fabs(m[8]));
    if (std::fabs(m[1] - m[3]) > tol || std::fabs(m[2] - m[6]) > tol || std::fabs(m[5] - m[7]) > tol)
      return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: %s is not symmetric", names[k]);
    const double d2 = m[0] * m[4] - m[1] * m[3];
    const double d3 = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(m[0] > 0.0 && d2 > 0.0 && d3 > 0.0)) return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: %s is not positive definite", names[k]);
  }
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(b->torque_chaser[i]) || !std::isfinite(b->torque_target[i])) return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: torque is not finite");
  if (!(b->rtol > 0.0 && std::isfinite(b->rtol) && b->atol > 0.0 && std::isfinite(b->atol)))
    return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: rtol and atol must be positive");
  const bool closed = closed_form_applies(b->inertia_chaser, b->torque_chaser) && closed_form_applies(b->inertia_target, b->torque_target);
  if (b->integrator == RDV_INTEGRATOR_EXACT && !closed)
    return fail(RDV_ERR_BAD_PARAMS, "RdvRigidBody: the closed-form integrator needs inertia = c * Identity and zero torque for both bodies");
  *general = b->integrator == RDV_INTEGRATOR_RK45 || !closed;
  return RDV_OK;
}
static void apply_body(const RdvRigidBody& b, DevParams& dev) {   // a validated body -> the kGeneral block of `dev`
  const double* tensors[2] = {b.inertia_chaser, b.inertia_target};
  const double* torques[2] = {b.torque_chaser, b.torque_target};
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i < 9; ++i) dev.body_inertia[k][i] = tensors[k][i];
    (void)invert3(tensors[k], dev.body_inv_inertia[k]);
    for (int i = 0; i < 3; ++i) dev.body_torque[k][i] = torques[k][i];
  }
  dev.rk_rtol = b.rtol; dev.rk_atol = b.atol;
  // per body: RK45 where the closed form does not apply to THAT body (or was asked for): a tri-axial target leaves the chaser on it
  for (int k = 0; k < 2; ++k) dev.body_general[k] = (b.integrator == RDV_INTEGRATOR_RK45 || !closed_form_applies(tensors[k], torques[k])) ? 1 : 0;
  if (b.integrator == RDV_INTEGRATOR_EXACT) dev.body_general[0] = dev.body_general[1] = 0;
}
// a handle's derived block for the parameters `p`: the thresholds, the handle's acos table, its rigid body
static void derive_block(const RdvEnvBatch* h, const RdvParams& p, DevParams& dev) {
  derive_params(p, dev);
  dev.acos_table = h->acos_table;
  apply_body(h->body, dev);
}
// one group's derived block -> its place in the device table, ordered on `s` (params_kernel, as upload_params)
static int upload_group(RdvEnvBatch* h, int32_t g, hipStream_t s) {
  hipLaunchKernelGGL(params_kernel, dim3(1), dim3(kWave), 0, s, h->group_dev[(size_t)g], const_cast<DevParams*>(h->group_table.params) + g);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}
int rdv_set_rigid_body(rdv_handle h, const RdvRigidBody* b, void* stream) {
  RDV_CHECK_HANDLE(h);
  bool general = false;
  if (int rc = validate_rigid_body(b, &general)) return rc;
  if (general && h->n_groups)
    return fail(RDV_ERR_BAD_PARAMS, "rdv_set_rigid_body: a general rigid body (RK45) cannot be combined with parameter groups: this handle has %d groups "
                                    "(rdv_set_param_groups with n_groups = 0 returns it to one block)", h->n_groups);
  DeviceGuard guard(h->device);
  h->body = *b; h->general = general;
  apply_body(h->body, h->dev);
  for (int32_t g = 0; g < h->n_groups; ++g) {
    apply_body(h->body, h->group_dev[(size_t)g]);
    if (int rc = upload_group(h, g, static_cast<hipStream_t>(stream))) return rc;
  }
  return upload_params(h, static_cast<hipStream_t>(stream));
}
int rdv_get_rigid_body(rdv_handle h, RdvRigidBody* out) {
  RDV_CHECK_HANDLE(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_rigid_body: null output");
  *out = h->body;
  return RDV_OK;
}

int rdv_set_params(rdv_handle h, const RdvParams* p, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_params: this handle has %d parameter groups: use rdv_set_group_params (or rdv_set_param_groups)", h->n_groups);
  if (int rc = rdv_params_validate(p)) return rc;
  DeviceGuard guard(h->device);
  h->params = *p; derive_block(h, *p, h->dev);
  h->prepared_ok = false; h->step_slots_ok = false;   // nominal state / ranges may have changed: what a reset returns is no longer what the slots hold
  // ... and the same on the device, ordered on `stream`: a graph recorded earlier holds a persistent kernel without the prepare launch that
  // prepared_ok asks for, and a tag says only which episode a slot belongs to, not which parameters drew it.  A tag of 0 never equals
  // episode + 1, so the kernels' own guard refills every slot from the new block before its first use (capturable: a memset node).
  RDV_HIP(hipMemsetAsync(h->prep_tag, 0, (size_t)h->n * sizeof(uint32_t), static_cast<hipStream_t>(stream)));
  return upload_params(h, static_cast<hipStream_t>(stream));
}
int rdv_get_params(rdv_handle h, RdvParams* out) {
  RDV_CHECK_HANDLE(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_params: null output");
  if (h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_params: this handle has %d parameter groups: use rdv_get_group_params", h->n_groups);
  *out = h->params;
  return RDV_OK;
}
int rdv_seed(rdv_handle h, uint64_t seed) {
  RDV_CHECK_HANDLE(h);
  h->seed = seed; h->fresh = true; h->prepared_ok = false; h->step_slots_ok = false;
  return RDV_OK;
}
#ifdef RDV_STAMPS
int rdv_debug_set_stamps(rdv_handle h, unsigned long long* stamps) {   // diagnostic build only; [n_waves_launched][8]
  RDV_CHECK_HANDLE(h);
  h->stamps = stamps;
  return RDV_OK;
}
#endif
int rdv_set_kernel_variant(rdv_handle h, int variant) {
  RDV_CHECK_HANDLE(h);
  if (variant != RDV_VARIANT_AUTO && variant != RDV_VARIANT_FUSED && variant != RDV_VARIANT_SPLIT && variant != RDV_VARIANT_FUSED_INLANE &&
      variant != RDV_VARIANT_FUSED_TILES)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_kernel_variant: bad variant %d", variant);
  h->variant = variant;
  return RDV_OK;
}
int rdv_set_reset_tape(rdv_handle h, const double* tape, int32_t depth) {
  RDV_CHECK_HANDLE(h);
  if ((tape == nullptr) != (depth <= 0)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_reset_tape: tape and depth must both be set or both be empty");
  h->tape = tape; h->tape_depth = tape ? depth : 0;
  h->prepared_ok = false; h->step_slots_ok = false;   // the slots hold states of the previous reset source
  return RDV_OK;
}

int rdv_reset(rdv_handle h, const uint8_t* mask, float* obs_out, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int fresh = (h->fresh && !mask) ? 1 : 0;
  if (h->fresh && mask) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_reset: the first reset after create/seed must cover all envs (mask = NULL)");
  StepArgs A;
  base_args(h, A);
  if (h->n_groups) launch_reset_groups(h->storage == RDV_STORAGE_F32, grid_for(h->n), s, h->group_table, A, mask, obs_out, fresh);
  else with_storage(h->storage, [&](auto st) { hipLaunchKernelGGL(reset_kernel<decltype(st)>, grid_for(h->n), dim3(kBlock), 0, s, h->dev_params, A, mask, obs_out, fresh); });
  RDV_HIP(hipGetLastError());
  if (fresh) h->prepared_ok = h->step_slots_ok = true;   // reset_kernel refills the slot of every env it resets: after a full reset all are current
  h->fresh = false;
  return RDV_OK;
}

int rdv_step(rdv_handle h, const float* actions, const RdvStepOut* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!actions || !out || !out->obs || !out->reward || !out->done)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step: actions, obs, reward and done are required");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step: call rdv_reset first (state is undefined until reset(), as in the reference)");
  RDV_CHECK_FAULT(h);
  if (misaligned(actions, 8) || misaligned(out->obs, 16))   // 8-byte loads of action rows, 16-byte stores of observation rows
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step: actions must be 8-byte aligned (any row of a [K,N,6] tape is) and obs 16-byte aligned");
  if (out->diag && misaligned(out->diag, 8)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step: diag must be 8-byte aligned");
  DeviceGuard guard(h->device);
  StepArgs A;
  base_args(h, A);
  A.actions = actions;
  A.obs = out->obs; A.reward = out->reward; A.done = out->done; A.terminal_obs = out->terminal_obs;
  A.episode_return = out->episode_return; A.episode_length = out->episode_length; A.done_reason = out->done_reason;
  A.diag = out->diag; A.eval = out->eval;
  if (A.eval && misaligned(A.eval, 8)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step: eval must be 8-byte aligned");
#ifdef RDV_STAMPS
  A.stamps = h->stamps;
#endif
  hipStream_t s = static_cast<hipStream_t>(stream);
  // general rigid bodies run on the fused layout only (their integrator is a per-lane adaptive loop: no fixed phase to split), as do
  // the evaluator-diagnostics build and the first step after rdv_set_state (kRaw)
  const bool raw = h->raw_state && !h->general;   // (the RK45 kernels integrate the quaternion as given, like the reference)
  h->raw_state = false;
  const bool split = !A.diag && !A.eval && !h->general && !raw && !h->n_groups && (h->variant == RDV_VARIANT_SPLIT || (h->variant == RDV_VARIANT_AUTO && h->n <= kSplitAutoMaxEnvs));
  // every launch records the kernel's name, as spelled here, on the handle (host only: rdv_debug_last_kernel)
#define RDV_K_SPLIT(ST, B) step_kernel_split<ST, B>
#define RDV_K_PARTS(ST, B) step_kernel_parts<ST, B>
#define RDV_K_FUSED(ST, B) step_kernel<ST, B>
#define RDV_K_RAW(ST, B) step_kernel<ST, B, false, true>
  const bool f32 = h->storage == RDV_STORAGE_F32, dg = A.diag != nullptr || A.eval != nullptr;   // either one: the evaluator build
  const bool slots = split && f32 && h->on_done == RDV_ON_DONE_RESET && (h->split_form < 0 ? split_slots_by_size(h->n) : h->split_form != 0);
  if (slots) {
    // the slot form (rdv_step.h): the same instantiation by name — the third template argument has a default — with one refill workgroup
    // appended per step workgroup
    if (int rc = ensure_step_slots(h, s)) return rc;
    const unsigned step_wgs = (unsigned)((h->n + kSplitEnvs - 1) / kSplitEnvs);
    // ... and the target form of the slot form (step_kernel_split_target): the same grid, the same name on the handle
    const bool target = h->split_form < 0 ? split_target_by_size(h->n) : h->split_form >= 2;
    // ... and its observation form (step_kernel_split_obs), likewise
    const bool obs = target && (h->split_form < 0 ? split_obs_by_size(h->n) : h->split_form == 3);
    if (obs) hipLaunchKernelGGL((step_kernel_split_obs<float>), dim3(2u * step_wgs), dim3(kSplitBlock), 0, s, RDV_HOT_ARGS(A, h->dev_params), A);
    else if (target) hipLaunchKernelGGL((step_kernel_split_target<float>), dim3(2u * step_wgs), dim3(kSplitBlock), 0, s, RDV_HOT_ARGS(A, h->dev_params), A);
    else hipLaunchKernelGGL((step_kernel_split<float, true, true>), dim3(2u * step_wgs), dim3(kSplitBlock), 0, s, RDV_HOT_ARGS(A, h->dev_params), A);
    h->last_kernel = "step_kernel_split<float, true>";
  } else if (split) {
    const dim3 grid((unsigned)((h->n + kSplitEnvs - 1) / kSplitEnvs));
    const dim3 block(kSplitBlock);
    const bool all = h->on_done != RDV_ON_DONE_HALT;   // no halted envs: every lane runs the transition, the inputs travel together (advance_all)
    RDV_LAUNCH_BY(h->last_kernel, f32, all, RDV_K_SPLIT, grid, block, s, RDV_HOT_ARGS(A, h->dev_params), A);
  } else {
    dim3 grid = grid_for(h->n), block(kBlock);
    { static const int forced = [] { const char* x = getenv("RDV_STREAM_ROWS"); return x ? atoi(x) : -1; }();   // diagnostics
      A.stream_rows = forced >= 0 ? (forced ? 1 : 0) : 1; }
    { static const int forced = [] { const char* x = getenv("RDV_STAGGER"); return x ? atoi(x) : -1; }();     // diagnostics: units of 512 cycles
      A.stagger = forced >= 0 ? forced : stagger_by_size(h->n); }
    if (h->xcd_order == 1 || (h->xcd_order < 0 && xcd_order_by_size(h->n))) {
      A.xcd_per = (int32_t)((grid.x + 7) / 8);
      grid = dim3((unsigned)A.xcd_per * 8u);   // up to 7 padding workgroups, which find no envs
    }
    if (h->n_groups) {
      // rdv_groups.hip: every workgroup binds the block of its tile's group.  The evaluator build and the first step after rdv_set_state run
      // the in-lane form, everything else — whichever variant was asked for — the reset-by-part form
      if (raw || dg) h->last_kernel = launch_step_groups_lane(f32, dg, raw, grid, s, h->group_table, A);
      else h->last_kernel = launch_step_groups(f32, h->on_done != RDV_ON_DONE_HALT, grid, s, h->group_table, A);
    } else if (h->general) {
      // rdv_general.hip: a general TARGET is integrated on partner waves beside the chaser half of the transition (step_kernel_general);
      // the evaluator build, and a general chaser beside the reference's target, run the fused per-lane form
      h->last_kernel = launch_step_general(f32, dg, h->dev.body_general[1] != 0 && h->split_general != 0, h->n, grid, s, h->dev_params, A);
    } else if (raw) {
      RDV_LAUNCH_BY(h->last_kernel, f32, dg, RDV_K_RAW, grid, block, s, RDV_HOT_ARGS(A, h->dev_params), A);
    } else if (!dg && h->variant != RDV_VARIANT_FUSED_INLANE) {
      const bool tiles = h->variant == RDV_VARIANT_FUSED_TILES && h->on_done != RDV_ON_DONE_HALT && h->tape_depth == 0;   // (halted envs skip the transition, a reset tape is a test device: step_kernel_parts)
      if (tiles) {
        // the tile loop: a grid of kTilesPerCU workgroups per CU (a multiple of 8: one eighth per XCD), never more than there are tiles
        unsigned g = h->tiles_grid ? (unsigned)h->tiles_grid : (unsigned)(h->n_cus * kTilesPerCU + 7) / 8u * 8u;
        const unsigned need = A.xcd_per ? (unsigned)A.xcd_per * 8u : grid.x;
        if (g > need) g = need;
        grid = dim3(g);
        h->last_kernel = launch_step_tiles(f32, grid, s, h->dev_params, A);
      } else {
        const bool all = h->on_done != RDV_ON_DONE_HALT;   // (see the split branch)
        RDV_LAUNCH_BY(h->last_kernel, f32, all, RDV_K_PARTS, grid, block, s, RDV_HOT_ARGS(A, h->dev_params), A);
      }
    } else {
      RDV_LAUNCH_BY(h->last_kernel, f32, dg, RDV_K_FUSED, grid, block, s, RDV_HOT_ARGS(A, h->dev_params), A);
    }
  }
#undef RDV_K_RAW
#undef RDV_K_FUSED
#undef RDV_K_PARTS
#undef RDV_K_SPLIT
  RDV_HIP(hipGetLastError());
  if (h->on_done == RDV_ON_DONE_RESET) h->prepared_ok = false;   // the step kernels reset in registers: the slots of the persistent kernels lag behind now
  h->step_slots_ok = slots;   // (the slot form leaves the slots of the episodes that ended to the next launch's refill: enough for itself, not for the persistent kernels)
  return RDV_OK;
}

int rdv_step_many(rdv_handle h, const float* actions, int32_t n_steps, const RdvStepOut* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (n_steps <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step_many: n_steps must be positive (got %d)", n_steps);
  if (!actions || !out || !out->obs || !out->reward || !out->done)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step_many: actions, obs, reward and done are required");
  if (out->terminal_obs || out->episode_return || out->episode_length || out->diag || out->eval)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step_many: terminal_obs, episode_return, episode_length, diag and eval are outputs of rdv_step only");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step_many: call rdv_reset first (state is undefined until reset(), as in the reference)");
  RDV_CHECK_FAULT(h);
  if (misaligned(actions, 8) || misaligned(out->obs, 16))
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_step_many: actions must be 8-byte aligned and obs 16-byte aligned");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->general || h->n_groups) {
    // General rigid bodies and parameter groups: n_steps launches of rdv_step on `stream` (the definition of this call's results, used as its
    // implementation): the per-lane RK45 does not fit the persistent kernel's register budget without scratch (round 2: 60 spilled
    // dwords per lane), and a step is bound by the integrator, not by the launch boundary this call exists to remove.
    const int64_t n = h->n;
    for (int32_t k = 0; k < n_steps; ++k) {
      RdvStepOut so;
      std::memset(&so, 0, sizeof so);
      so.obs = obs_row_target(h, out->obs, k);
      so.reward = out->reward + (int64_t)k * n; so.done = out->done + (int64_t)k * n;
      so.done_reason = out->done_reason ? out->done_reason + (int64_t)k * n : nullptr;
      if (int rc = rdv_step(h, actions + (int64_t)k * n * RDV_ACT_DIM, &so, stream)) return rc;
      if (int rc = obs_row_flush(h, out->obs, k, s)) return rc;
    }
    return RDV_OK;
  }
  h->raw_state = false;   // the kernel integrates injected (unnormalised) quaternions itself
  if (int rc = ensure_prepared(h, s)) return rc;
  StepManyArgs A;
  fill_batch_fields(A, h);
  A.actions = actions; A.obs = out->obs; A.reward = out->reward; A.done = out->done; A.done_reason = out->done_reason; A.n_steps = n_steps;
  const dim3 grid((unsigned)((h->n + kManyEnvs - 1) / kManyEnvs)), block(kManyBlock);
  with_storage(h->storage, [&](auto st) {
    using ST = decltype(st);
    hipLaunchKernelGGL((step_many_kernel<ST, false>), grid, block, many_lds_bytes<ST>(), s, h->dev_params, A);
  });
  h->last_kernel = h->storage == RDV_STORAGE_F32 ? "step_many_kernel<float, false>" : "step_many_kernel<double, false>";
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

static int access(rdv_handle h, int what, const double* in, double* out, float* out_f32, void* stream) {
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->n_groups) launch_access_groups(h->storage == RDV_STORAGE_F32, grid_for(h->n), s, h->group_table, h->ws, h->n, h->cs, what, in, out, out_f32);
  else with_storage(h->storage, [&](auto st) { hipLaunchKernelGGL(access_kernel<decltype(st)>, grid_for(h->n), dim3(kBlock), 0, s, h->dev, h->ws, h->n, h->cs, what, in, out, out_f32); });
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

int rdv_set_state(rdv_handle h, const double* states, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!states) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_state: null states");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_state: call rdv_reset first (monte_carlo.py:106 resets before overwriting the state)");
  h->raw_state = true;
  return access(h, ACC_SET_STATE, states, nullptr, nullptr, stream);
}
int rdv_get_state(rdv_handle h, double* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_state: null output");
  return access(h, ACC_GET_STATE, nullptr, out, nullptr, stream);
}
// ---- snapshot / restore of the whole batch (state, bookkeeping, flags, episode counters, statistics): a 64-byte header, then
// the chunk arrays and the statistics slots, which are one contiguous region at the start of the workspace
struct SnapshotHeader {
  uint32_t magic, version;
  int64_t n_envs;
  int32_t storage, reserved;
  int64_t payload_bytes;
  uint64_t pad[4];
};
static_assert(sizeof(SnapshotHeader) == 64, "snapshot header layout");
static constexpr uint32_t kSnapMagic = 0x52445653u;   // "RDVS"
__global__ void snapshot_header_kernel(const SnapshotHeader hd, SnapshotHeader* dst) { if (threadIdx.x == 0) *dst = hd; }
static inline int64_t snapshot_payload(const RdvEnvBatch* h) { return workspace_layout(h->n, h->storage).params; }   // chunks + statistics: everything in front of the parameter block

int64_t rdv_snapshot_bytes(rdv_handle h) {
  if (!h || h->magic != kMagic) return -1;
  return (int64_t)sizeof(SnapshotHeader) + snapshot_payload(h);
}
int rdv_snapshot(rdv_handle h, void* dst, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!dst) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_snapshot: null destination");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_snapshot: nothing to save before the first rdv_reset");
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  SnapshotHeader hd;
  std::memset(&hd, 0, sizeof hd);
  hd.magic = kSnapMagic; hd.version = 1; hd.n_envs = h->n; hd.storage = h->storage; hd.payload_bytes = snapshot_payload(h);
  hipLaunchKernelGGL(snapshot_header_kernel, dim3(1), dim3(kWave), 0, s, hd, static_cast<SnapshotHeader*>(dst));
  RDV_HIP(hipGetLastError());
  RDV_HIP(hipMemcpyAsync(static_cast<char*>(dst) + sizeof(SnapshotHeader), h->ws, (size_t)hd.payload_bytes, hipMemcpyDeviceToDevice, s));
  return RDV_OK;
}
int rdv_restore(rdv_handle h, const void* src, int64_t src_bytes, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!src) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_restore: null source");
  if (src_bytes < (int64_t)sizeof(SnapshotHeader)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_restore: %lld bytes cannot hold a snapshot header", (long long)src_bytes);
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = refuse_in_capture("rdv_restore", s)) return rc;
  SnapshotHeader hd;   // the header is validated on the host: this call synchronises `stream`
  RDV_HIP(hipMemcpyAsync(&hd, src, sizeof hd, hipMemcpyDeviceToHost, s));
  if (int rc = read_fault_word(h, s)) return rc;   // (it synchronises anyway)
  RDV_CHECK_FAULT(h);
  if (hd.magic != kSnapMagic || hd.version != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_restore: the buffer does not start with a snapshot header");
  if (hd.n_envs != h->n || hd.storage != h->storage)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_restore: snapshot of %lld envs with storage %d, this batch has %lld envs with storage %d",
                (long long)hd.n_envs, hd.storage, (long long)h->n, h->storage);
  if (hd.payload_bytes != snapshot_payload(h) || src_bytes < (int64_t)sizeof(SnapshotHeader) + hd.payload_bytes)
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_restore: the buffer holds %lld bytes, the snapshot needs %lld", (long long)src_bytes,
                (long long)(sizeof(SnapshotHeader) + snapshot_payload(h)));
  RDV_HIP(hipMemcpyAsync(h->ws, static_cast<const char*>(src) + sizeof(SnapshotHeader), (size_t)hd.payload_bytes, hipMemcpyDeviceToDevice, s));
  // the halted flags of the snapshot mean something to a HALT handle only: elsewhere every kernel steps the env on (include/rdv.h)
  if (h->on_done != RDV_ON_DONE_HALT)
    if (int rc = access(h, ACC_CLEAR_HALTED, nullptr, nullptr, nullptr, stream)) return rc;
  h->fresh = false;
  h->raw_state = true;      // the snapshot may have been taken right after rdv_set_state
  h->prepared_ok = false; h->step_slots_ok = false;   // the episode counters changed: the slots are re-derived before the next launch that uses them
  return RDV_OK;
}

int rdv_get_aux(rdv_handle h, double* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_aux: null output");
  return access(h, ACC_GET_AUX, nullptr, out, nullptr, stream);
}
int rdv_observe(rdv_handle h, float* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_observe: null output");
  return access(h, ACC_OBSERVE, nullptr, nullptr, out, stream);
}
int rdv_diagnose(rdv_handle h, double* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_diagnose: null output");
  return access(h, ACC_DIAGNOSE, nullptr, out, nullptr, stream);
}

int rdv_eval_begin(rdv_handle h, double* eval, void* stream) {
  RDV_CHECK_HANDLE(h);
  RDV_CHECK_FAULT(h);
  if (!eval) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_eval_begin: null accumulators");
  if (h->fresh) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_eval_begin: call rdv_reset first");
  return access(h, ACC_EVAL_BEGIN, nullptr, eval, nullptr, stream);
}
// the evaluation summary of envs [first, last) (whole waves, or up to the batch's end): rdv_eval_summary, rdv_eval_group_summary
static int eval_summary_of(const char* who, rdv_handle h, const double* eval, RdvEvalSummary* out, int64_t first, int64_t last, void* stream) {
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = refuse_in_capture(who, s)) return rc;
  if (h->n_groups) launch_eval_summary_groups(h->storage == RDV_STORAGE_F32, grid_for(h->n), s, h->group_table, h->ws, h->n, h->cs, eval, h->eval_partial);
  else with_storage(h->storage, [&](auto st) { hipLaunchKernelGGL(eval_summary_kernel<decltype(st)>, grid_for(h->n), dim3(kBlock), 0, s, h->dev, h->ws, h->n, h->cs, eval, h->eval_partial); });
  RDV_HIP(hipGetLastError());
  const size_t waves = (size_t)((h->n + kWave - 1) / kWave);
  h->host_eval.resize(waves * EV_SLOTS);
  RDV_HIP(hipMemcpyAsync(h->host_eval.data(), h->eval_partial, waves * EV_SLOTS * sizeof(double), hipMemcpyDeviceToHost, s));
  if (int rc = read_fault_word(h, s)) return rc;
  RDV_CHECK_FAULT(h);
  double t[EV_SLOTS] = {0};
  for (size_t w = (size_t)(first / kWave); w < (size_t)((last + kWave - 1) / kWave); ++w)      // fixed order: reproducible sums
    for (int j = 0; j <= EV_N; ++j) t[j] += h->host_eval[w * EV_SLOTS + j];
  const double m = t[EV_N];
  std::memset(out, 0, sizeof *out);
  out->episodes = (int64_t)m;
  out->ep_rew = t[EV_REW] / m; out->ep_len = t[EV_LEN] / m; out->ep_dist = t[EV_DIST] / m; out->ep_delta_v = t[EV_DV] / m;
  out->ep_delta_w = t[EV_DW] / m; out->ep_success = t[EV_SUCC] / m; out->ep_collision_percentage = t[EV_COLLP] / m;
  out->ep_time_of_first_collision = t[EV_TFIRST_N] > 0 ? t[EV_TFIRST] / t[EV_TFIRST_N] : -1.0;        // :274-282
  out->ep_min_pos_error = t[EV_MINPOS_N] > 0 ? t[EV_MINPOS] / t[EV_MINPOS_N] : -1.0;
  out->ep_avg_att_error = t[EV_AVGATT] / m;
  out->pct_collided_episodes = t[EV_NCOLL] / m * 100.0; out->pct_successful_episodes = t[EV_NSUCC] / m * 100.0;   // :270-271
  return RDV_OK;
}
int rdv_eval_summary(rdv_handle h, const double* eval, RdvEvalSummary* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!eval || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_eval_summary: null accumulators / output");
  return eval_summary_of("rdv_eval_summary", h, eval, out, 0, h->n, stream);
}
int rdv_eval_group_summary(rdv_handle h, int32_t group, const double* eval, RdvEvalSummary* out, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!eval || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_eval_group_summary: null accumulators / output");
  if (group < 0 || group >= h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_eval_group_summary: group %d of %d", group, h->n_groups);
  return eval_summary_of("rdv_eval_group_summary", h, eval, out, h->group_start[(size_t)group], h->group_start[(size_t)group + 1], stream);
}

// the statistics slots -> the host (synchronises `stream`, reads the device error word; reset: zeroes them behind the copy)
static int fetch_slots(RdvEnvBatch* h, int reset, hipStream_t s) {
  const size_t bytes = h->host_slots.size() * sizeof(uint64_t);
  RDV_HIP(hipMemcpyAsync(h->host_slots.data(), h->stats, bytes, hipMemcpyDeviceToHost, s));
  return read_fault_word(h, s, reset ? bytes : 0);
}
// the slots of waves [first, last) summed in ascending order: the sums are reproducible run to run
static void sum_slots(const RdvEnvBatch* h, size_t first, size_t last, RdvStats* out) {
  std::memset(out, 0, sizeof *out);
  for (size_t w = first; w < last; ++w) {
    const uint64_t* sl = h->host_slots.data() + w * kStatWords;
    const double* sd = reinterpret_cast<const double*>(sl);
    out->env_steps += sl[ST_STEPS]; out->episodes += sl[ST_EPISODES]; out->successes += sl[ST_SUCCESS]; out->collisions += sl[ST_COLLIDED];
    for (int r = 0; r < 4; ++r) out->reasons[r] += sl[ST_REASON0 + r];
    out->sum_length += (double)sl[ST_SUM_LEN]; out->sum_return += sd[ST_SUM_RET]; out->sum_delta_v += sd[ST_SUM_DV]; out->sum_delta_w += sd[ST_SUM_DW];
  }
}
int rdv_get_stats(rdv_handle h, RdvStats* out, int reset, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_stats: null output");
  DeviceGuard guard(h->device);
  if (int rc = refuse_in_capture("rdv_get_stats", static_cast<hipStream_t>(stream))) return rc;
  if (int rc = fetch_slots(h, reset, static_cast<hipStream_t>(stream))) return rc;
  sum_slots(h, 0, h->host_slots.size() / kStatWords, out);
  return rdv_device_error_code(h->device_error);   // RDV_OK unless a kernel of this handle reported a fault (the statistics are filled either way)
}
int rdv_get_group_stats(rdv_handle h, RdvStats* out, int reset, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_group_stats: null output");
  if (!h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_group_stats: this handle has no parameter groups (rdv_get_stats)");
  DeviceGuard guard(h->device);
  if (int rc = refuse_in_capture("rdv_get_group_stats", static_cast<hipStream_t>(stream))) return rc;
  if (int rc = fetch_slots(h, reset, static_cast<hipStream_t>(stream))) return rc;
  // a group begins on a 256-env boundary, so its waves are a range of slots: the range a stand-alone handle of that group would sum
  for (int32_t g = 0; g < h->n_groups; ++g)
    sum_slots(h, (size_t)(h->group_start[(size_t)g] / kWave), (size_t)((h->group_start[(size_t)g + 1] + kWave - 1) / kWave), out + g);
  return rdv_device_error_code(h->device_error);
}

// ---- parameter groups ----------------------------------------------------------------------------------------------
int rdv_param_groups_check(int64_t n_envs, int32_t n_groups, const int64_t* sizes) {
  if (n_groups < 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: n_groups = %d: a grouped batch has at least group 0", n_groups);
  if (!sizes) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: null group sizes");
  // the tile table holds one int32 group index per 256 envs; a group has at least one env, so no more groups than envs fit either
  if ((int64_t)n_groups > n_envs) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: group %d does not fit: %d groups for %lld envs", n_groups - 1, n_groups, (long long)n_envs);
  int64_t at = 0;
  for (int32_t g = 0; g < n_groups; ++g) {
    if (sizes[g] <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: group %d has size %lld: sizes must be positive", g, (long long)sizes[g]);
    if (g + 1 < n_groups && sizes[g] % kGroupTile != 0)
      return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: group %d has size %lld: every group but the last must be a multiple of %d envs "
                                            "(a workgroup of 256 envs shares one parameter block)", g, (long long)sizes[g], kGroupTile);
    at += sizes[g];
    if (at > n_envs) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: group %d ends at env %lld, the batch has %lld envs", g, (long long)at, (long long)n_envs);
  }
  if (at != n_envs) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_check: group %d (the last) ends at env %lld, the batch has %lld envs", n_groups - 1, (long long)at, (long long)n_envs);
  return RDV_OK;
}
int rdv_param_groups_validate(const RdvParams* params, int32_t n_groups) {
  if (!params || n_groups < 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_param_groups_validate: null params / no group");
  for (int32_t g = 0; g < n_groups; ++g)
    if (rdv_params_validate(params + g)) {
      char why[400];
      std::snprintf(why, sizeof why, "%s", g_err);
      return fail(RDV_ERR_BAD_PARAMS, "parameters of group %d: %s", g, why);
    }
  return RDV_OK;
}
int rdv_set_param_groups(rdv_handle h, const RdvParams* params, const int64_t* sizes, int32_t n_groups, void* stream) {
  RDV_CHECK_HANDLE(h);
  {
    DeviceGuard guard(h->device);
    if (int rc = refuse_in_capture("rdv_set_param_groups", static_cast<hipStream_t>(stream))) return rc;
  }
  if (n_groups == 0) {   // back to the handle's single block (the side allocation stays until rdv_destroy or the next grouping)
    if (h->n_groups) h->prepared_ok = h->step_slots_ok = false;
    h->n_groups = 0;
    return RDV_OK;
  }
  if (h->general) return fail(RDV_ERR_BAD_PARAMS, "rdv_set_param_groups: parameter groups cannot be combined with a general rigid body (RK45): this handle has one (rdv_set_rigid_body)");
  if (int rc = rdv_param_groups_check(h->n, n_groups, sizes)) return rc;
  if (int rc = rdv_param_groups_validate(params, n_groups)) return rc;
  DeviceGuard guard(h->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t tiles = (h->n + kGroupTile - 1) / kGroupTile, entries = align_up(tiles, 8);   // the XCD order pads the grid to a multiple of 8
  const size_t block_bytes = (size_t)align_up((int64_t)n_groups * (int64_t)sizeof(DevParams), 256), bytes = block_bytes + (size_t)entries * sizeof(int32_t);
  if (bytes > h->group_mem_bytes) {
    h->n_groups = 0;
    if (h->group_mem) { RDV_HIP(hipStreamSynchronize(s)); (void)hipFree(h->group_mem); h->group_mem = nullptr; h->group_mem_bytes = 0; }
    hipError_t err = hipMalloc(&h->group_mem, bytes);
    if (err != hipSuccess) { (void)hipGetLastError(); h->group_mem = nullptr; return fail(RDV_ERR_OUT_OF_MEMORY, "rdv_set_param_groups: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err)); }
    h->group_mem_bytes = bytes;
  }
  h->group_params.assign(params, params + n_groups);
  h->group_dev.resize((size_t)n_groups);
  h->group_start.assign((size_t)n_groups + 1, 0);
  for (int32_t g = 0; g < n_groups; ++g) {
    derive_block(h, params[g], h->group_dev[(size_t)g]);
    h->group_start[(size_t)g + 1] = h->group_start[(size_t)g] + sizes[g];
  }
  const std::vector<int32_t> table = tile_table(sizes, n_groups, kGroupTile, entries);
  char* const base = static_cast<char*>(h->group_mem);
  // the copies leave pageable host memory that this call owns: ordered on `stream`, and waited for before it returns
  RDV_HIP(hipMemcpyAsync(base, h->group_dev.data(), (size_t)n_groups * sizeof(DevParams), hipMemcpyHostToDevice, s));
  RDV_HIP(hipMemcpyAsync(base + block_bytes, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  RDV_HIP(hipStreamSynchronize(s));
  h->group_table.params = reinterpret_cast<const DevParams*>(base);
  h->group_table.tile_group = reinterpret_cast<const int32_t*>(base + block_bytes);
  h->n_groups = n_groups;
  h->prepared_ok = false; h->step_slots_ok = false;
  return RDV_OK;
}
int rdv_set_group_params(rdv_handle h, int32_t group, const RdvParams* p, void* stream) {
  RDV_CHECK_HANDLE(h);
  if (group < 0 || group >= h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_set_group_params: group %d of %d", group, h->n_groups);
  if (int rc = rdv_params_validate(p)) return rc;
  DeviceGuard guard(h->device);
  h->group_params[(size_t)group] = *p; derive_block(h, *p, h->group_dev[(size_t)group]);
  // (prepared_ok stays as it is, unlike in rdv_set_params: only the persistent kernels read the slots, a grouped handle never launches one —
  // rdv_step_many and rdv_rollout run the rdv_step loop — and every way out of the grouped state, rdv_set_param_groups, clears the flag)
  return upload_group(h, group, static_cast<hipStream_t>(stream));
}
int rdv_get_group_params(rdv_handle h, int32_t group, RdvParams* out) {
  RDV_CHECK_HANDLE(h);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_group_params: null output");
  if (group < 0 || group >= h->n_groups) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_get_group_params: group %d of %d", group, h->n_groups);
  *out = h->group_params[(size_t)group];
  return RDV_OK;
}
int32_t rdv_num_groups(rdv_handle h) { return (h && h->magic == kMagic) ? h->n_groups : -1; }

}  // extern "C"

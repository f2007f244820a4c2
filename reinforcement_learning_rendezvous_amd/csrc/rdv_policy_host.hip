// rdv_policy_host.hip — the host side of the policy handles of include/rdv.h: RdvPolicyNet (rdv_host.h) and its create / destroy / act /
// value / set-weights entry points, policy sets, the recurrent policy and its sets (rdv_lstm_*), rdv_mlp_spec_*, rdv_lstm_spec_check, rdv_gae,
// rdv_rollout_advantages, rdv_ppo_*, rdv_ppo_mlp_* (the set form rdv_ppo_mlp_set_* among them), rdv_lstm_ppo_* (rdv_lstm_ppo_set_adam_step among them), rdv_ppo_set_adam_step, rdv_policy_get_block, and policy_act_step, the act half of rdv_rollout's act + step loop (the loop, which owns the env handle, is in
// rdv_hip.hip).  HOST ONLY: no kernel is defined here; they are reached through the launch functions of the headers below (shipped_*,
// mlp_*, sets_*, lstm_*, gae_launch, ppo_launch, ppo_set_launch, ppo_mlp_launch, lstm_ppo_launch, ppo_adam_launch, lstm_adam_launch), so an edit to an argument check recompiles no kernel.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_policy_mlp.h"
#include "rdv_policy_lstm.h"
#include "rdv_policy_sets.h"
#include "rdv_advantages.h"
#include "rdv_ppo.h"
#include "rdv_ppo_mlp.h"
#include "rdv_ppo_lstm.h"
#include "rdv_ppo_adam.h"
#include "rdv_ppo_lstm_adam.h"
#include "rdv_host.h"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>

using namespace rdv;

// the shipped architecture, which IS rdv_policy_create / rdv_critic_create: same block, same kernels, the persistent rollout kernel
static const RdvMlpSpec kDefaultMlpSpec = {2, {64, 64, 0, 0}, RDV_ACT_TANH, 0};
static bool is_default_spec(const RdvMlpSpec& spec) { return std::memcmp(&spec, &kDefaultMlpSpec, sizeof(RdvMlpSpec)) == 0; }
static bool is_shipped(const RdvMlpSpec* spec) {
#ifndef RDV_MLP_GENERAL_DEFAULT   // (diagnostic build, tools/mlp_arch_time.py: the shipped architecture through the general kernel, to time the two side by side)
  return is_default_spec(*spec);
#else
  return false;
#endif
}
static bool all_finite(const float* w, int count) {
  for (int i = 0; i < count; ++i) if (!std::isfinite(w[i])) return false;
  return true;
}
// The layers of a trunk (first input width in0, then `spec`, then out_dim), l = 0 .. n_hidden: null pointers (kNull), non-finite weights
// (kFinite), or both layer by layer.  `where`: how the message names layer l — "layer %d", "trunk layer %d", "layer %d of member %d" (g).
enum { kNull = 1, kFinite = 2 };
static int check_layers(int what, const char* who, const char* where, int g, int in0, const RdvMlpSpec& spec, int out_dim,
                        const float* const* weights, const float* const* biases) {
  const int L = spec.n_hidden;
  char layer[48];
  for (int l = 0; l <= L; ++l) {
    const int in_w = l == 0 ? in0 : spec.hidden[l - 1], out_w = l < L ? spec.hidden[l] : out_dim;
    const bool null = (what & kNull) && (!weights[l] || !biases[l]);
    if (!null && (!(what & kFinite) || all_finite(weights[l], out_w * in_w))) continue;
    std::snprintf(layer, sizeof layer, where, l, g);
    return null ? fail(RDV_ERR_INVALID_ARGUMENT, "%s: null weights or biases of %s", who, layer)
                : fail(RDV_ERR_BAD_PARAMS, "%s: non-finite weight in %s", who, layer);
  }
  return RDV_OK;
}
// one network's parameter block, as the kernels of its architecture read it
static void pack_block(bool shipped, const RdvMlpSpec& spec, int out_dim, const float* const* weights, const float* const* biases, const float* log_std,
                       std::vector<float>& packed) {
  if (shipped) pack_policy_weights(weights[0], biases[0], weights[1], biases[1], weights[2], biases[2], log_std, out_dim, packed);
  else pack_mlp_weights(spec, out_dim, weights, biases, log_std, packed);
}

// what rdv_policy_destroy frees, and a constructor that fails half-way
static void free_policy(RdvPolicyNet* p) {
  (void)hipFree(p->weights);
  if (p->lstm_state) (void)hipFree(p->lstm_state);
  if (p->staging) (void)hipHostFree(p->staging);
  for (hipEvent_t ev : p->staged) if (ev) (void)hipEventDestroy(ev);
  p->magic = 0; delete p;
}
// THE constructor of a policy handle on `device` (the caller's DeviceGuard holds it).  `blocks`: the n_members packed blocks back to back,
// uploaded to the `weights` allocation; `table` (a set: non-null): the tile table, placed behind them at the next multiple of 256 bytes.
// lstm_hidden != 0: the state allocation for `rows` rows, zeroed, every row's start pending.  Otherwise the dynamic-LDS limits of exactly
// the kernels the handle will run are raised above the 64 KiB default (72 KiB for the shipped architecture, up to 90,752 B for 4 x 64).
static int make_policy(const char* who, int device, int out_dim, const RdvMlpSpec& spec, bool shipped, int32_t n_members, int64_t rows,
                       int32_t lstm_hidden, const std::vector<float>& blocks, const std::vector<int32_t>* table, rdv_policy* out) {
  RdvPolicyNet* p = new (std::nothrow) RdvPolicyNet();
  if (!p) return fail(RDV_ERR_OUT_OF_MEMORY, "%s: host allocation failed", who);
  p->device = device; p->out_dim = out_dim; p->spec = spec; p->shipped_arch = shipped; p->block_floats = (int)(blocks.size() / (size_t)n_members);
  p->n_members = n_members; p->rows = rows; p->lstm_hidden = lstm_hidden;
  const size_t block_bytes = blocks.size() * sizeof(float), table_at = (size_t)align_up((int64_t)block_bytes, 256);
  hipError_t err = hipMalloc(&p->weights, table ? table_at + table->size() * sizeof(int32_t) : block_bytes);
  if (err == hipSuccess) err = hipMemcpy(p->weights, blocks.data(), block_bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && table) {
    p->tile_member = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p->weights) + table_at);
    err = hipMemcpy(const_cast<int32_t*>(p->tile_member), table->data(), table->size() * sizeof(int32_t), hipMemcpyHostToDevice);
  }
  if (lstm_hidden) {
    const size_t state_floats = (size_t)rows * (size_t)lstm_hidden, obs_floats = ((size_t)rows * kPolIn + 3) & ~(size_t)3;
    const size_t bytes = (4 * state_floats + obs_floats) * sizeof(float) + (size_t)rows;
    if (err == hipSuccess) err = hipMalloc(&p->lstm_state, bytes);
    if (err == hipSuccess) err = hipMemset(p->lstm_state, 0, bytes);
    if (err == hipSuccess) {
      p->lstm_h = p->lstm_state; p->lstm_c = p->lstm_h + state_floats; p->lstm_h_next = p->lstm_c + state_floats;
      p->lstm_c_tmp = p->lstm_h_next + state_floats; p->lstm_obs_tmp = p->lstm_c_tmp + state_floats;
      p->lstm_pending = reinterpret_cast<uint8_t*>(p->lstm_obs_tmp + obs_floats);
      err = hipMemset(p->lstm_pending, 1, (size_t)rows);
    }
  } else {   // a set of one member runs the plain kernels on its one block; larger sets the set kernels
    if (err == hipSuccess) err = shipped ? shipped_raise_lds_limit() : mlp_raise_lds_limit();
    if (err == hipSuccess && table) err = sets_raise_lds_limit(shipped);
  }
  if (err != hipSuccess) { (void)hipGetLastError(); free_policy(p); return fail(err == hipErrorOutOfMemory ? RDV_ERR_OUT_OF_MEMORY : RDV_ERR_HIP, "%s: %s", who, hipGetErrorString(err)); }
  *out = p;
  return RDV_OK;
}

// A 17-64-64-out_dim tanh MLP of the checkpoint (out_dim <= 6) as a parameter block on the device
static int create_mlp(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                      const float* log_std, int out_dim, int device, rdv_policy* out) {
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_create / rdv_critic_create: null argument");
  if (int rc = check_device("rdv_policy_create", device)) return rc;
  DeviceGuard guard(device);
  if (!all_finite(w1, kPolHid * kPolIn) || !all_finite(w2, kPolHid * kPolHid) || !all_finite(w3, out_dim * kPolHid))
    return fail(RDV_ERR_BAD_PARAMS, "rdv_policy_create: non-finite weight");
  const float *const w[3] = {w1, w2, w3}, *const b[3] = {b1, b2, b3};
  std::vector<float> packed;
  pack_block(true, kDefaultMlpSpec, out_dim, w, b, log_std, packed);
  return make_policy("rdv_policy_create", device, out_dim, kDefaultMlpSpec, true, 1, 0, 0, packed, nullptr, out);
}
static int create_mlp_spec(const RdvMlpSpec* spec, const float* const* weights, const float* const* biases, const float* log_std,
                           int out_dim, int device, rdv_policy* out) {
  if (!spec || !weights || !biases || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_create_mlp / rdv_critic_create_mlp: null argument");
  if (int rc = rdv_mlp_spec_check(spec)) return rc;
  if (int rc = check_layers(kNull, "rdv_policy_create_mlp / rdv_critic_create_mlp", "layer %d", 0, kPolIn, *spec, out_dim, weights, biases)) return rc;
  if (is_shipped(spec)) return create_mlp(weights[0], biases[0], weights[1], biases[1], weights[2], biases[2], log_std, out_dim, device, out);
  if (int rc = check_device("rdv_policy_create_mlp", device)) return rc;
  DeviceGuard guard(device);
  if (int rc = check_layers(kFinite, "rdv_policy_create_mlp", "layer %d", 0, kPolIn, *spec, out_dim, weights, biases)) return rc;
  std::vector<float> packed;
  pack_block(false, *spec, out_dim, weights, biases, log_std, packed);
  return make_policy("rdv_policy_create_mlp", device, out_dim, *spec, false, 1, 0, 0, packed, nullptr, out);
}

// ---- refreshing a handle's weights (a learner's optimiser step): the block is packed on the host as at creation and copied into the
// handle's device allocation from a pinned buffer of the handle's own, on the caller's stream
// block `member` of the handle <- packed (of the handle's block size, or refused), ordered on `stream`.  The pinned staging has one slot and one event per member, so refreshing
// all members back to back never waits on the host for another member's copy, only for the previous refresh of the same member.
static int upload_block(rdv_policy p, const char* who, int32_t member, const std::vector<float>& packed, void* stream) {
  if ((int)packed.size() != p->block_floats) return fail(RDV_ERR_HIP, "%s: the packed block has %d floats, the handle's %d", who, (int)packed.size(), p->block_floats);
  DeviceGuard guard(p->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = refuse_in_capture(who, s, "(the staging buffer is reused by the next call)")) return rc;
  const size_t floats = (size_t)p->block_floats, bytes = floats * sizeof(float);
  if (!p->staging) {
    RDV_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->staging), bytes * (size_t)p->n_members, hipHostMallocDefault));
    p->staged.assign((size_t)p->n_members, nullptr);
  }
  hipEvent_t& ev = p->staged[(size_t)member];
  if (!ev) RDV_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  else RDV_HIP(hipEventSynchronize(ev));   // the previous refresh of this member has left its slot (usually long ago)
  float* slot = p->staging + floats * (size_t)member;
  std::memcpy(slot, packed.data(), bytes);
  RDV_HIP(hipMemcpyAsync(p->weights + floats * (size_t)member, slot, bytes, hipMemcpyHostToDevice, s));
  RDV_HIP(hipEventRecord(ev, s));
  return RDV_OK;
}
// one network's host arrays checked against the handle's spec, packed, and uploaded as block `member`
static int refresh_member(rdv_policy p, const char* who, int32_t member, const float* const* weights, const float* const* biases, const float* log_std, void* stream) {
  if (!weights || !biases) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null weights_host or biases_host", who);
  const bool actor = p->out_dim == kPolOut;
  if (actor && !log_std) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: log_std_host is required for an actor", who);
  if (!actor && log_std) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: log_std_host must be null for a critic (rdv_critic_create)", who);
  if (int rc = check_layers(kNull, who, "layer %d", 0, kPolIn, p->spec, p->out_dim, weights, biases)) return rc;
  if (int rc = check_layers(kFinite, who, "layer %d", 0, kPolIn, p->spec, p->out_dim, weights, biases)) return rc;
  std::vector<float> packed;
  pack_block(p->shipped_arch, p->spec, p->out_dim, weights, biases, log_std, packed);
  return upload_block(p, who, member, packed, stream);
}

// ---- policy sets (csrc/rdv_policy_sets.h): n_members networks of one spec, member g owning sizes[g] consecutive rows
// *rows <- the sum of a set's sizes, judged by the rule of parameter groups (a size that is not positive or would overflow ends the sum, and is named against a count nothing exceeds)
static int set_rows(const char* who, int32_t n_members, const int64_t* sizes, int64_t* rows) {
  if (n_members < 1) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n_members = %d: a set has at least member 0", who, n_members);
  constexpr int64_t kMostRows = INT64_MAX / 2;
  *rows = 0;
  for (int32_t g = 0; g < n_members && *rows >= 0; ++g) *rows = (sizes[g] > 0 && sizes[g] <= kMostRows - *rows) ? *rows + sizes[g] : -1;
  return rdv_param_groups_check(*rows < 0 ? kMostRows : *rows, n_members, sizes);
}
// all <- the members' blocks back to back, each exactly the bytes of a stand-alone handle (pack_one(g, packed): member g's), all of one size
template <class PackOne> static int pack_members(const char* who, int32_t n_members, PackOne pack_one, std::vector<float>& all) {
  std::vector<float> packed;
  for (int32_t g = 0; g < n_members; ++g) {
    pack_one(g, packed);
    if (g && packed.size() * (size_t)g != all.size()) return fail(RDV_ERR_HIP, "%s: member %d packs to %zu floats, member 0 to %zu", who, g, packed.size(), all.size() / (size_t)g);
    all.insert(all.end(), packed.begin(), packed.end());
  }
  return RDV_OK;
}
static int create_set(const char* who, const RdvMlpSpec* spec, int32_t n_members, const int64_t* sizes, const float* const* const* weights,
                      const float* const* const* biases, const float* const* log_std, int out_dim, int device, rdv_policy* out) {
  if (!spec || !sizes || !weights || !biases || !out || (out_dim == kPolOut && !log_std)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (int rc = rdv_mlp_spec_check(spec)) return rc;
  int64_t rows = 0;
  if (int rc = set_rows(who, n_members, sizes, &rows)) return rc;
  for (int32_t g = 0; g < n_members; ++g) {
    if (!weights[g] || !biases[g] || (out_dim == kPolOut && !log_std[g])) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null weights, biases or log_std of member %d", who, g);
    if (int rc = check_layers(kNull | kFinite, who, "layer %d of member %d", g, kPolIn, *spec, out_dim, weights[g], biases[g])) return rc;
  }
  if (int rc = check_device(who, device)) return rc;
  DeviceGuard guard(device);
  const bool shipped = is_shipped(spec);
  std::vector<float> all;
  const auto pack_one = [&](int32_t g, std::vector<float>& packed) { pack_block(shipped, *spec, out_dim, weights[g], biases[g], out_dim == kPolOut ? log_std[g] : nullptr, packed); };
  if (int rc = pack_members(who, n_members, pack_one, all)) return rc;
  const std::vector<int32_t> table = tile_table(sizes, n_members, kSetTile, (rows + kSetTile - 1) / kSetTile);
  return make_policy(who, device, out_dim, *spec, shipped, n_members, rows, 0, all, &table, out);
}

// The forward kernels of a feed-forward handle on n rows (checked against p->rows by the callers), the one place that chooses them: the set
// forms for more than one member (each 256-row tile reads its member's block; a critic's flat row r belongs to env r mod rows: n / rows row
// blocks), else the general MLP kernels, else the shipped pair; by out_dim the actor (out = clipped actions) or the critic (out = values).
static int launch_forward(rdv_policy p, const float* obs, float* out, int64_t n, int deterministic, uint64_t seed, uint64_t counter,
                          uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  const bool critic = p->out_dim == 1, set = p->n_members > 1;
  const int act = p->spec.activation, bf = p->block_floats;
  const float* W = p->weights;
  if (set && critic) sets_launch_value(p->shipped_arch, act, W, bf, p->tile_member, obs, out, p->rows, n / p->rows, s);
  else if (set) sets_launch_act(p->shipped_arch, act, W, bf, p->tile_member, obs, out, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s);
  else if (critic) (p->shipped_arch ? shipped_launch_value : mlp_launch_value)(act, W, bf, obs, out, n, s);
  else (p->shipped_arch ? shipped_launch_act : mlp_launch_act)(act, W, bf, obs, out, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- GAE (csrc/rdv_advantages.h)
// gamma, gae_lambda and the sizes: what rdv_gae and rdv_rollout_advantages check alike, before any device is looked at
static int check_gae_scalars(const char* who, int32_t n_steps, int64_t n, double gamma, double gae_lambda) {
  if (n_steps <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n_steps must be positive (got %d)", who, n_steps);
  if (n <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n must be positive (got %lld)", who, (long long)n);
  if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: gamma must be in [0, 1] (got %g)", who, gamma);
  if (!std::isfinite(gae_lambda) || gae_lambda < 0.0 || gae_lambda > 1.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: gae_lambda must be in [0, 1] (got %g)", who, gae_lambda);
  return RDV_OK;
}
static int launch_gae(const float* reward, const uint8_t* done, const float* values, const float* last_value, int32_t n_steps, int64_t n,
                      double gamma, double gae_lambda, float* advantages, float* returns, hipStream_t s) {
  // (diagnostics only: RDV_GAE_DEPTH = 2 | 4 | 8 | 16 picks the kernel's prefetch depth, for tools/gae_time.py; results do not depend on it)
  const char* x = getenv("RDV_GAE_DEPTH");
  const int d = x ? atoi(x) : 0;
  gae_launch(reward, done, values, last_value, n_steps, n, (float)gamma, (float)(gamma * gae_lambda), advantages, returns,
             (d == 2 || d == 4 || d == 8 || d == 16) ? d : 0, s);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- the recurrent policy (csrc/rdv_policy_lstm.h): one LSTM layer in front of an RdvMlpSpec trunk, the state owned by the handle
// null pointers and finiteness of a recurrent network's host arrays (the spec has been checked)
static int check_lstm_arrays(const char* who, int H, const RdvMlpSpec& trunk, int out_dim, const float* w_ih, const float* w_hh, const float* b_ih,
                             const float* b_hh, const float* const* weights, const float* const* biases, const float* log_std) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !weights || !biases) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (out_dim == kPolOut && !log_std) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: log_std_host is required for an actor", who);
  if (out_dim != kPolOut && log_std) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: log_std_host must be null for a critic", who);
  if (int rc = check_layers(kNull, who, "trunk layer %d", 0, H, trunk, out_dim, weights, biases)) return rc;
  if (!all_finite(w_ih, 4 * H * kPolIn) || !all_finite(w_hh, 4 * H * H) || !all_finite(b_ih, 4 * H) || !all_finite(b_hh, 4 * H))
    return fail(RDV_ERR_BAD_PARAMS, "%s: non-finite LSTM weight", who);
  return check_layers(kFinite, who, "trunk layer %d", 0, H, trunk, out_dim, weights, biases);
}
static int create_lstm(const char* who, const RdvLstmSpec* spec, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                       const float* const* weights, const float* const* biases, const float* log_std, int out_dim, int64_t n_rows, int device,
                       rdv_policy* out) {
  if (!spec || !out) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (int rc = rdv_lstm_spec_check(spec)) return rc;
  const int H = spec->hidden_size;
  if (n_rows <= 0 || n_rows > (int64_t)1 << 31) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n_rows = %lld must be in 1..2^31", who, (long long)n_rows);
  if (int rc = check_lstm_arrays(who, H, spec->trunk, out_dim, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std)) return rc;
  if (int rc = check_device(who, device)) return rc;
  DeviceGuard guard(device);
  std::vector<float> packed;
  pack_lstm_weights(H, spec->trunk, out_dim, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std, packed);
  return make_policy(who, device, out_dim, spec->trunk, false, 1, n_rows, H, packed, nullptr, out);
}
// ---- recurrent policy sets: n_members recurrent networks of one RdvLstmSpec, member g owning sizes[g] consecutive rows; the handle owns
// the state and the pending flags of all rows.  The order of work: the spec, the sizes, every member's arrays, then the device.
static int create_lstm_set(const char* who, const RdvLstmSpec* spec, int32_t n_members, const int64_t* sizes, const float* const* w_ih,
                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* const* const* weights,
                           const float* const* const* biases, const float* const* log_std, int out_dim, int device, rdv_policy* out) {
  if (!spec || !sizes || !w_ih || !w_hh || !b_ih || !b_hh || !weights || !biases || !out || (out_dim == kPolOut && !log_std))
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (int rc = rdv_lstm_spec_check(spec)) return rc;
  int64_t rows = 0;
  if (int rc = set_rows(who, n_members, sizes, &rows)) return rc;
  if (rows > (int64_t)1 << 31) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the sizes sum to %lld rows, which must be in 1..2^31", who, (long long)rows);
  const int H = spec->hidden_size;
  char member[96];
  for (int32_t g = 0; g < n_members; ++g) {
    std::snprintf(member, sizeof member, "%s: member %d", who, g);
    if (int rc = check_lstm_arrays(member, H, spec->trunk, out_dim, w_ih[g], w_hh[g], b_ih[g], b_hh[g], weights[g], biases[g],
                                   out_dim == kPolOut ? log_std[g] : nullptr)) return rc;
  }
  if (int rc = check_device(who, device)) return rc;
  DeviceGuard guard(device);
  std::vector<float> all;
  const auto pack_one = [&](int32_t g, std::vector<float>& packed) { pack_lstm_weights(H, spec->trunk, out_dim, w_ih[g], w_hh[g], b_ih[g], b_hh[g], weights[g], biases[g], out_dim == kPolOut ? log_std[g] : nullptr, packed); };
  if (int rc = pack_members(who, n_members, pack_one, all)) return rc;
  const std::vector<int32_t> table = tile_table(sizes, n_members, kSetTile, (rows + kSetTile - 1) / kSetTile);
  return make_policy(who, device, out_dim, spec->trunk, false, n_members, rows, H, all, &table, out);
}
// one recurrent network's host arrays checked against the handle's spec, packed, and uploaded as block `member`
static int refresh_lstm_member(rdv_policy p, const char* who, int32_t member, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                               const float* const* weights, const float* const* biases, const float* log_std, void* stream) {
  if (int rc = check_lstm_arrays(who, p->lstm_hidden, p->spec, p->out_dim, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std)) return rc;
  std::vector<float> packed;
  pack_lstm_weights(p->lstm_hidden, p->spec, p->out_dim, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std, packed);
  return upload_block(p, who, member, packed, stream);
}
#define RDV_CHECK_LSTM(p, who) \
  RDV_CHECK_POLICY(p);         \
  if (!(p)->lstm_hidden) return fail(RDV_ERR_INVALID_ARGUMENT, who ": this handle is not a recurrent policy (rdv_lstm_policy_create / rdv_lstm_critic_create)")

// one step of a recurrent handle on `s`: the cell (flags: u8 [rows] or nullptr), then the trunk; commit: the state advances (the
// pending flags are the caller's business).  The caller's DeviceGuard holds the device; the arguments have been checked.
static int launch_lstm(rdv_policy p, const float* obs, const uint8_t* flags, float* out, float* raw_actions, float* log_prob, bool commit,
                       int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, hipStream_t s) {
  const int32_t* table = p->n_members > 1 ? p->tile_member : nullptr;   // a set of one member runs the plain kernels on its one block
  lstm_launch_cell(p->lstm_hidden, p->weights, p->block_floats, table, obs, flags, p->lstm_h, p->lstm_c, p->lstm_h_next,
                   commit ? p->lstm_c : p->lstm_c_tmp, p->rows, s);
  RDV_HIP(hipGetLastError());
  lstm_launch_trunk(p->spec.activation, p->out_dim == 1, p->weights, p->block_floats, table, p->lstm_h_next, commit ? p->lstm_h : nullptr, out,
                    p->rows, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s);
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

int rdv::policy_act_step(rdv_policy p, int32_t t, const float* obs, const uint8_t* done, float* actions, int64_t n, int deterministic, uint64_t seed,
                         uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  if (!p->lstm_hidden) return launch_forward(p, obs, actions, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s);
  return launch_lstm(p, obs, t == 0 ? p->lstm_pending : done + (int64_t)(t - 1) * n, actions, raw_actions, log_prob, true, deterministic, seed, counter,
                     env_id_offset, s);
}

// rdv_rollout_advantages with a recurrent critic: n_steps committing steps in time order, one non-committing step on last_obs (GAE follows)
static int values_lstm(rdv_policy critic, const RdvRolloutOut* rows, int32_t n_steps, int64_t n, const RdvAdvantageOut* out, hipStream_t s) {
  const bool aligned = (n & 3) == 0;                                   // row t of rows->obs is 16-byte aligned if and only if n % 4 == 0
  for (int32_t t = 0; t < n_steps; ++t) {
    const float* obs_t = rows->obs + (int64_t)t * n * RDV_OBS_DIM;
    if (!aligned) {
      RDV_HIP(hipMemcpyAsync(critic->lstm_obs_tmp, obs_t, (size_t)n * RDV_OBS_DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
      obs_t = critic->lstm_obs_tmp;
    }
    if (int rc = launch_lstm(critic, obs_t, t == 0 ? critic->lstm_pending : rows->done + (int64_t)(t - 1) * n, out->values + (int64_t)t * n, nullptr, nullptr, true, 1, 0, 0, 0, s)) return rc;
  }
  const uint8_t* last_done = rows->done + (int64_t)(n_steps - 1) * n;
  if (int rc = launch_lstm(critic, rows->last_obs, last_done, out->last_value, nullptr, nullptr, false, 1, 0, 0, 0, s)) return rc;
  RDV_HIP(hipMemcpyAsync(critic->lstm_pending, last_done, (size_t)n, hipMemcpyDeviceToDevice, s));
  return RDV_OK;
}

extern "C" {

int rdv_policy_create(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                      const float* log_std, int device, rdv_policy* out) {
  if (!log_std) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_create: null argument");
  return create_mlp(w1, b1, w2, b2, w3, b3, log_std, kPolOut, device, out);
}
int rdv_critic_create(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                      int device, rdv_policy* out) {
  return create_mlp(w1, b1, w2, b2, w3, b3, nullptr, 1, device, out);
}

// ---- other architectures (RdvMlpSpec): csrc/rdv_policy_mlp.h
int rdv_mlp_spec_default(RdvMlpSpec* out_host) {
  if (!out_host) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_mlp_spec_default: null argument");
  *out_host = kDefaultMlpSpec;
  return RDV_OK;
}

int rdv_mlp_spec_check(const RdvMlpSpec* spec) {
  if (!spec) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_mlp_spec_check: null spec");
  if (spec->n_hidden < 1 || spec->n_hidden > RDV_MLP_MAX_HIDDEN)
    return fail(RDV_ERR_INVALID_ARGUMENT, "RdvMlpSpec: n_hidden = %d is not in 1..%d", spec->n_hidden, RDV_MLP_MAX_HIDDEN);
  for (int l = 0; l < RDV_MLP_MAX_HIDDEN; ++l) {
    const int wd = spec->hidden[l];
    if (l < spec->n_hidden ? (wd != 16 && wd != 32 && wd != 64) : wd != 0)
      return fail(RDV_ERR_INVALID_ARGUMENT, l < spec->n_hidden ? "RdvMlpSpec: hidden[%d] = %d is not 16, 32 or 64" : "RdvMlpSpec: hidden[%d] = %d beyond n_hidden must be 0", l, wd);
  }
  if (spec->activation != RDV_ACT_TANH && spec->activation != RDV_ACT_RELU && spec->activation != RDV_ACT_SIGMOID)
    return fail(RDV_ERR_INVALID_ARGUMENT, "RdvMlpSpec: activation = %d is not an RdvActivation (0 tanh, 1 relu, 2 sigmoid)", spec->activation);
  if (spec->reserved != 0) return fail(RDV_ERR_INVALID_ARGUMENT, "RdvMlpSpec: reserved = %d must be 0", spec->reserved);
  return RDV_OK;
}

int rdv_policy_create_mlp(const RdvMlpSpec* spec_host, const float* const* weights_host, const float* const* biases_host,
                          const float* log_std_host, int device, rdv_policy* out) {
  if (!log_std_host) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_create_mlp: null argument");
  return create_mlp_spec(spec_host, weights_host, biases_host, log_std_host, kPolOut, device, out);
}
int rdv_critic_create_mlp(const RdvMlpSpec* spec_host, const float* const* weights_host, const float* const* biases_host,
                          int device, rdv_policy* out) {
  return create_mlp_spec(spec_host, weights_host, biases_host, nullptr, 1, device, out);
}

int rdv_policy_get_spec(rdv_policy p, RdvMlpSpec* out_host) {
  RDV_CHECK_POLICY(p);
  if (!out_host) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_get_spec: null argument");
  *out_host = p->spec;
  return RDV_OK;
}

int rdv_policy_set_weights(rdv_policy p, const float* const* weights, const float* const* biases, const float* log_std, void* stream) {
  RDV_CHECK_POLICY(p);
  if (p->lstm_hidden) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_set_weights: this handle is a recurrent policy (rdv_lstm_policy_create): use rdv_lstm_set_weights");
  if (p->n_members > 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_set_weights: this handle is a policy set of %d members: refresh one member with rdv_policy_set_member_weights", p->n_members);
  return refresh_member(p, "rdv_policy_set_weights", 0, weights, biases, log_std, stream);
}

int rdv_policy_set_member_weights(rdv_policy p, int32_t member, const float* const* weights, const float* const* biases, const float* log_std, void* stream) {
  RDV_CHECK_POLICY(p);
  if (p->lstm_hidden) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_set_member_weights: this handle is a recurrent policy (rdv_lstm_policy_create): use rdv_lstm_set_weights");
  if (member < 0 || member >= p->n_members) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_set_member_weights: member %d of %d", member, p->n_members);
  return refresh_member(p, "rdv_policy_set_member_weights", member, weights, biases, log_std, stream);
}

int rdv_policy_set_create(const RdvMlpSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* const* weights_host,
                          const float* const* const* biases_host, const float* const* log_std_host, int device, rdv_policy* out) {
  return create_set("rdv_policy_set_create", spec_host, n_members, sizes_host, weights_host, biases_host, log_std_host, kPolOut, device, out);
}
int rdv_critic_set_create(const RdvMlpSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* const* weights_host,
                          const float* const* const* biases_host, int device, rdv_policy* out) {
  return create_set("rdv_critic_set_create", spec_host, n_members, sizes_host, weights_host, biases_host, nullptr, 1, device, out);
}
int32_t rdv_policy_num_members(rdv_policy p) { return (p && p->magic == kPolicyMagic) ? p->n_members : -1; }
int64_t rdv_policy_num_rows(rdv_policy p) { return (p && p->magic == kPolicyMagic) ? p->rows : -1; }

int rdv_policy_destroy(rdv_policy p) {
  RDV_CHECK_POLICY(p);
  DeviceGuard guard(p->device);
  (void)hipDeviceSynchronize();
  free_policy(p);
  return RDV_OK;
}

int rdv_policy_act(rdv_policy p, const float* obs, float* actions, int64_t n, int deterministic, uint64_t seed, uint64_t counter,
                   uint64_t env_id_offset, void* stream) {
  RDV_CHECK_POLICY(p);
  if (p->lstm_hidden) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_act: this handle is a recurrent policy (rdv_lstm_policy_create): use rdv_lstm_act, which carries the state");
  if (p->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_act: this handle is a critic (rdv_critic_create)");
  if (!obs || !actions || n <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_act: obs, actions and a positive n are required");
  if (misaligned(obs, 16) || misaligned(actions, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_act: obs and actions must be 16-byte aligned");
  if (p->rows && n != p->rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_act: n = %lld, the policy set owns %lld rows", (long long)n, (long long)p->rows);
  DeviceGuard guard(p->device);
  return launch_forward(p, obs, actions, n, deterministic, seed, counter, env_id_offset, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int rdv_policy_value(rdv_policy p, const float* obs, float* values, int64_t n, void* stream) {
  RDV_CHECK_POLICY(p);
  if (p->lstm_hidden) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_value: this handle is a recurrent policy (rdv_lstm_critic_create): use rdv_lstm_value, which carries the state");
  if (p->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_value: this handle is an actor (rdv_policy_create)");
  if (!obs || !values || n <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_value: obs, values and a positive n are required");
  if (misaligned(obs, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_value: obs must be 16-byte aligned");
  if (p->rows && n % p->rows != 0) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_policy_value: n = %lld is not a multiple of the %lld rows the critic set owns", (long long)n, (long long)p->rows);
  DeviceGuard guard(p->device);
  return launch_forward(p, obs, values, n, 1, 0, 0, 0, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int rdv_gae(const float* reward, const uint8_t* done, const float* values, const float* last_value, int32_t n_steps, int64_t n,
            double gamma, double gae_lambda, float* advantages, float* returns, int device, void* stream) {
  const struct { const void* p; const char* name; } ptrs[] = {{reward, "reward"}, {done, "done"}, {values, "values"}, {last_value, "last_value"},
                                                              {advantages, "advantages"}, {returns, "returns"}};
  for (const auto& a : ptrs) if (!a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_gae: %s is null", a.name);
  if (int rc = check_gae_scalars("rdv_gae", n_steps, n, gamma, gae_lambda)) return rc;
  if (int rc = check_device("rdv_gae", device)) return rc;
  DeviceGuard guard(device);
  return launch_gae(reward, done, values, last_value, n_steps, n, gamma, gae_lambda, advantages, returns, static_cast<hipStream_t>(stream));
}

int rdv_lstm_spec_check(const RdvLstmSpec* spec) {
  if (!spec) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_spec_check: null spec");
  if (!lstm_hidden_ok(spec->hidden_size))
    return fail(RDV_ERR_BAD_PARAMS, "RdvLstmSpec: hidden_size = %d is not 32, 64, 128 or 256 (lstm_hidden_size)", spec->hidden_size);
  if (spec->n_layers != 1)
    return fail(RDV_ERR_BAD_PARAMS, "RdvLstmSpec: n_layers = %d: one LSTM layer is served (n_lstm_layers = 1)", spec->n_layers);
  if (spec->shared != 0)
    return fail(RDV_ERR_BAD_PARAMS, "RdvLstmSpec: shared = %d: separate actor and critic LSTMs are served (shared_lstm = False, enable_critic_lstm = True)", spec->shared);
  if (spec->reserved != 0) return fail(RDV_ERR_BAD_PARAMS, "RdvLstmSpec: reserved = %d must be 0", spec->reserved);
  return rdv_mlp_spec_check(&spec->trunk);
}

int rdv_lstm_policy_create(const RdvLstmSpec* spec_host, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                           const float* const* weights_host, const float* const* biases_host, const float* log_std_host, int64_t n_rows,
                           int device, rdv_policy* out) {
  return create_lstm("rdv_lstm_policy_create", spec_host, w_ih, w_hh, b_ih, b_hh, weights_host, biases_host, log_std_host, kPolOut, n_rows, device, out);
}
int rdv_lstm_critic_create(const RdvLstmSpec* spec_host, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                           const float* const* weights_host, const float* const* biases_host, int64_t n_rows, int device, rdv_policy* out) {
  return create_lstm("rdv_lstm_critic_create", spec_host, w_ih, w_hh, b_ih, b_hh, weights_host, biases_host, nullptr, 1, n_rows, device, out);
}
int32_t rdv_lstm_hidden_size(rdv_policy p) { return (p && p->magic == kPolicyMagic) ? p->lstm_hidden : -1; }

int rdv_lstm_act(rdv_policy p, const float* obs, const uint8_t* episode_start, float* actions, float* raw_actions, float* log_prob, int64_t n,
                 int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_act");
  if (p->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_act: this handle is a critic (rdv_lstm_critic_create)");
  if (!obs || !actions) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_act: obs and actions are required");
  if (n != p->rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_act: n = %lld, the handle owns the state of %lld rows", (long long)n, (long long)p->rows);
  if (misaligned(obs, 16) || misaligned(actions, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_act: obs and actions must be 16-byte aligned");
  DeviceGuard guard(p->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = launch_lstm(p, obs, episode_start, actions, raw_actions, log_prob, true, deterministic ? 1 : 0, seed, counter, env_id_offset, s)) return rc;
  RDV_HIP(hipMemsetAsync(p->lstm_pending, 0, (size_t)p->rows, s));   // the state has moved past whatever start was pending
  return RDV_OK;
}

int rdv_lstm_value(rdv_policy p, const float* obs, const uint8_t* episode_start, float* values, int64_t n, int commit, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_value");
  if (p->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_value: this handle is an actor (rdv_lstm_policy_create)");
  if (!obs || !values) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_value: obs and values are required");
  if (n != p->rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_value: n = %lld, the handle owns the state of %lld rows", (long long)n, (long long)p->rows);
  if (misaligned(obs, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_value: obs must be 16-byte aligned");
  DeviceGuard guard(p->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = launch_lstm(p, obs, episode_start, values, nullptr, nullptr, commit != 0, 1, 0, 0, 0, s)) return rc;
  if (commit) RDV_HIP(hipMemsetAsync(p->lstm_pending, 0, (size_t)p->rows, s));
  return RDV_OK;
}

int rdv_lstm_get_state(rdv_policy p, float* h_out, float* c_out, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_get_state");
  if (!h_out || !c_out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_get_state: h_out and c_out are required");
  DeviceGuard guard(p->device);
  const size_t bytes = (size_t)p->rows * (size_t)p->lstm_hidden * sizeof(float);
  RDV_HIP(hipMemcpyAsync(h_out, p->lstm_h, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  RDV_HIP(hipMemcpyAsync(c_out, p->lstm_c, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return RDV_OK;
}

int rdv_lstm_set_state(rdv_policy p, const float* h, const float* c, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_set_state");
  if (!h || !c) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_set_state: h and c are required");
  DeviceGuard guard(p->device);
  const size_t bytes = (size_t)p->rows * (size_t)p->lstm_hidden * sizeof(float);
  RDV_HIP(hipMemcpyAsync(p->lstm_h, h, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  RDV_HIP(hipMemcpyAsync(p->lstm_c, c, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  RDV_HIP(hipMemsetAsync(p->lstm_pending, 0, (size_t)p->rows, static_cast<hipStream_t>(stream)));
  return RDV_OK;
}

int rdv_lstm_reset_state(rdv_policy p, const uint8_t* mask, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_reset_state");
  DeviceGuard guard(p->device);
  lstm_launch_reset(p->lstm_h, p->lstm_c, mask, p->rows, p->lstm_hidden, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

int rdv_lstm_set_weights(rdv_policy p, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* const* weights,
                         const float* const* biases, const float* log_std, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_set_weights");
  if (p->n_members > 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_set_weights: this handle is a recurrent policy set of %d members: refresh one member with rdv_lstm_set_member_weights", p->n_members);
  return refresh_lstm_member(p, "rdv_lstm_set_weights", 0, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std, stream);
}

int rdv_lstm_set_member_weights(rdv_policy p, int32_t member, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                const float* const* weights, const float* const* biases, const float* log_std, void* stream) {
  RDV_CHECK_LSTM(p, "rdv_lstm_set_member_weights");
  if (member < 0 || member >= p->n_members) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_lstm_set_member_weights: member %d of %d", member, p->n_members);
  return refresh_lstm_member(p, "rdv_lstm_set_member_weights", member, w_ih, w_hh, b_ih, b_hh, weights, biases, log_std, stream);
}

int rdv_lstm_policy_set_create(const RdvLstmSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* w_ih_host,
                               const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host,
                               const float* const* const* weights_host, const float* const* const* biases_host, const float* const* log_std_host,
                               int device, rdv_policy* out) {
  return create_lstm_set("rdv_lstm_policy_set_create", spec_host, n_members, sizes_host, w_ih_host, w_hh_host, b_ih_host, b_hh_host, weights_host,
                         biases_host, log_std_host, kPolOut, device, out);
}
int rdv_lstm_critic_set_create(const RdvLstmSpec* spec_host, int32_t n_members, const int64_t* sizes_host, const float* const* w_ih_host,
                               const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host,
                               const float* const* const* weights_host, const float* const* const* biases_host, int device, rdv_policy* out) {
  return create_lstm_set("rdv_lstm_critic_set_create", spec_host, n_members, sizes_host, w_ih_host, w_hh_host, b_ih_host, b_hh_host, weights_host,
                         biases_host, nullptr, 1, device, out);
}

int rdv_rollout_advantages(rdv_policy critic, const RdvRolloutOut* rows, int32_t n_steps, int64_t n, double gamma, double gae_lambda,
                           const RdvAdvantageOut* out, void* stream) {
  if (!rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: rows is null");
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: out is null");
  const struct { const void* p; const char* name; } ptrs[] = {{rows->obs, "rows->obs"}, {rows->reward, "rows->reward"}, {rows->done, "rows->done"},
                                                              {rows->last_obs, "rows->last_obs"}, {out->values, "out->values"}, {out->last_value, "out->last_value"},
                                                              {out->advantages, "out->advantages"}, {out->returns, "out->returns"}};
  for (const auto& a : ptrs) if (!a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: %s is null", a.name);
  if (int rc = check_gae_scalars("rdv_rollout_advantages", n_steps, n, gamma, gae_lambda)) return rc;
  RDV_CHECK_POLICY(critic);
  if (critic->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: this handle is an actor (rdv_policy_create)");
  if (critic->lstm_hidden && n != critic->rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: n = %lld, the recurrent critic owns the state of %lld rows", (long long)n, (long long)critic->rows);
  if (!critic->lstm_hidden && critic->rows && n != critic->rows) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: n = %lld, the critic set owns %lld rows", (long long)n, (long long)critic->rows);
  if (misaligned(rows->obs, 16) || misaligned(rows->last_obs, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_rollout_advantages: rows->obs and rows->last_obs must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DeviceGuard guard(critic->device);
  if (critic->lstm_hidden) {
    if (int rc = values_lstm(critic, rows, n_steps, n, out, s)) return rc;
  } else {
    // the critic at call time over the rows the actor saw, then over the observation after the last step: rdv_policy_value's own launches
    if (int rc = rdv_policy_value(critic, rows->obs, out->values, (int64_t)n_steps * n, stream)) return rc;
    if (int rc = rdv_policy_value(critic, rows->last_obs, out->last_value, n, stream)) return rc;
  }
  return launch_gae(rows->reward, rows->done, out->values, out->last_value, n_steps, n, gamma, gae_lambda, out->advantages, out->returns, s);
}

// ---- PPO minibatch gradients (csrc/rdv_ppo.h)
int64_t rdv_ppo_workspace_bytes(int64_t n) { return n > 0 ? ppo_workspace_bytes(n) : -1; }

int rdv_ppo_spec_check(const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec) {
  if (!actor_spec || !critic_spec) return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_ppo_spec_check: null %s", !actor_spec ? "actor_spec" : "critic_spec");
  if (int rc = rdv_mlp_spec_check(actor_spec)) return rc;
  if (int rc = rdv_mlp_spec_check(critic_spec)) return rc;
  const struct { const RdvMlpSpec* s; const char* name; } nets[] = {{actor_spec, "actor"}, {critic_spec, "critic"}};
  for (const auto& a : nets)
    if (!is_default_spec(*a.s))
      return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_ppo_loss_grad: the %s is not the shipped architecture (two hidden layers of 64, tanh): its gradients are not built", a.name);
  return RDV_OK;
}

static int check_ppo_coefficients(const char* who, double clip_range, double ent_coef, double vf_coef) {
  if (!std::isfinite(clip_range) || clip_range <= 0.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: clip_range must be finite and positive (got %g)", who, clip_range);
  if (!std::isfinite(ent_coef) || ent_coef < 0.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: ent_coef must be finite and not negative (got %g)", who, ent_coef);
  if (!std::isfinite(vf_coef) || vf_coef < 0.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: vf_coef must be finite and not negative (got %g)", who, vf_coef);
  return RDV_OK;
}
// The dynamic-LDS limit of one unit's PPO kernels (`raise`: ppo_raise_lds_limit, the plain and the set forms, or ppo_mlp_raise_lds_limit),
// once per device (`raised`: that unit's flags; a host-side attribute: no stream work); the caller's DeviceGuard holds `device`
static int raise_ppo_lds_limit(hipError_t (*raise)(), bool (&raised)[64], int device) {
  if (device >= 64 || !raised[device]) {
    RDV_HIP(raise());
    if (device < 64) raised[device] = true;
  }
  return RDV_OK;
}
static bool g_ppo_lds_raised[64], g_ppo_mlp_lds_raised[64];

extern "C++" {   // (two templates: RdvPpoOut / RdvPpoSetOut, and the entry points' own refusals as lambdas)
// What the three PPO entry points check of their rows, outputs and workspace ahead of everything else, in this order: rows, out and
// (set_form) counts_host non-null; every pointer the call needs (set_form: rows->indices too); n positive (the plain forms) or no
// negative count among the `members` counts and a positive one (set_form, which has no n); rows->rows; n against rows->rows where a
// plain form has no index vector; the two alignments.
template <class Out>
static int check_ppo_call(const char* who, const RdvPpoRows* rows, const Out* out, const void* workspace, bool set_form, int64_t n,
                          int32_t members, const int64_t* counts_host) {
  if (!rows) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows is null", who);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: out is null", who);
  if (set_form && !counts_host) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host is null", who);
  const struct { const void* p; const char* name; bool needed; } ptrs[] = {
      {rows->obs, "rows->obs", true}, {rows->actions, "rows->actions", true}, {rows->old_log_prob, "rows->old_log_prob", true},
      {rows->advantages, "rows->advantages", true}, {rows->returns, "rows->returns", true}, {rows->indices, "rows->indices", set_form},
      {out->actor_grad, "out->actor_grad", true}, {out->critic_grad, "out->critic_grad", true}, {out->scalars, "out->scalars", true},
      {workspace, "workspace", true}};
  for (const auto& a : ptrs) if (a.needed && !a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is null", who, a.name);
  if (set_form) {
    bool any = false;
    for (int32_t g = 0; g < members; ++g) {
      if (counts_host[g] < 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host[%d] = %lld is negative", who, g, (long long)counts_host[g]);
      any = any || counts_host[g] > 0;
    }
    if (!any) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host holds no positive count (%d member%s)", who, members, members == 1 ? "" : "s");
  } else if (n <= 0) {
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n must be positive (got %lld)", who, (long long)n);
  }
  if (rows->rows <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->rows must be positive (got %lld)", who, (long long)rows->rows);
  if (!set_form && !rows->indices && n > rows->rows)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: n = %lld exceeds rows->rows = %lld and rows->indices is null", who, (long long)n, (long long)rows->rows);
  if (misaligned(rows->obs, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->obs must be 16-byte aligned", who);
  if (misaligned(workspace, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  return RDV_OK;
}

// The refusals the three entry points make of their pair of handles, in this order: an invalid handle; per net a recurrent one and
// then what per_net(handle, name) refuses (the plain forms: a set); a swapped pair; what arch() refuses (an entry point's checks of the
// architecture, made ahead of the devices'); two devices.  W: how this entry point names its two handles, who creates them, and what it
// has not built for a recurrent set.
struct PpoHandleWords { bool set_form; const char *actor, *critic, *critic_creator, *actor_creator; const char* not_built = "its gradients are not built"; };
template <class PerNet, class Arch>
static int check_ppo_handles(const char* who, rdv_policy actor, rdv_policy critic, const PpoHandleWords& W, PerNet per_net, Arch arch) {
  RDV_CHECK_POLICY(actor);
  RDV_CHECK_POLICY(critic);
  const struct { rdv_policy p; const char* name; } nets[] = {{actor, W.actor}, {critic, W.critic}};
  for (const auto& a : nets) {
    if (a.p->lstm_hidden)
      return W.set_form ? fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is a recurrent policy or a recurrent set: %s", who, a.name, W.not_built)
                        : fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle is a recurrent policy: its gradients are not built", who, a.name);
    if (int rc = per_net(a.p, a.name)) return rc;
  }
  if (actor->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is a critic handle (%s): actor and critic are swapped", who, W.actor, W.critic_creator);
  if (critic->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is an actor handle (%s): actor and critic are swapped", who, W.critic, W.actor_creator);
  if (int rc = arch()) return rc;
  if (actor->device != critic->device) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s on device %d, %s on device %d", who, W.actor, actor->device, W.critic, critic->device);
  return RDV_OK;
}
}  // extern "C++"

int rdv_ppo_loss_grad(rdv_policy actor, rdv_policy critic, const RdvPpoRows* rows, int64_t n, double clip_range, double ent_coef, double vf_coef,
                      void* workspace, int64_t workspace_bytes, const RdvPpoOut* out, void* stream) {
  const char* who = "rdv_ppo_loss_grad";
  if (int rc = check_ppo_call(who, rows, out, workspace, false, n, 0, nullptr)) return rc;
  if (workspace_bytes < ppo_workspace_bytes(n))
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, n = %lld needs %lld (rdv_ppo_workspace_bytes)", who, (long long)workspace_bytes, (long long)n, (long long)ppo_workspace_bytes(n));
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  auto no_set = [&](rdv_policy p, const char* name) -> int {
    return p->n_members > 1 || p->rows ? fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle is a policy set: its gradients are not built", who, name) : RDV_OK;
  };
  auto shipped = [&]() -> int {
    if (int rc = rdv_ppo_spec_check(&actor->spec, &critic->spec)) return rc;
    return !actor->shipped_arch || !critic->shipped_arch ? fail(RDV_ERR_INVALID_ARGUMENT, "%s: the handles do not run the shipped kernels", who) : RDV_OK;
  };
  if (int rc = check_ppo_handles(who, actor, critic, {false, "actor", "critic", "rdv_critic_create", "rdv_policy_create"}, no_set, shipped)) return rc;
  DeviceGuard guard(actor->device);
  if (int rc = raise_ppo_lds_limit(ppo_raise_lds_limit, g_ppo_lds_raised, actor->device)) return rc;
  PpoLaunch a = {actor->weights, critic->weights, rows->obs, rows->actions, rows->old_log_prob, rows->advantages, rows->returns, rows->indices, n,
                 ppo_coefs(clip_range, ent_coef, vf_coef), static_cast<float*>(workspace), out->actor_grad, out->critic_grad, out->scalars, out->log_prob, out->values};
  ppo_launch(a, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- PPO minibatch gradients for every MLP architecture (csrc/rdv_ppo_mlp.h)
// what the two spec checks of the general calls share: both specs non-null, then rdv_mlp_spec_check's refusal of either under its name
static int check_spec_pair(const char* who, const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec, const char* actor, const char* critic) {
  if (!actor_spec || !critic_spec) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null %s", who, !actor_spec ? "actor_spec" : "critic_spec");
  const struct { const RdvMlpSpec* s; const char* name; } nets[] = {{actor_spec, actor}, {critic_spec, critic}};
  for (const auto& a : nets)
    if (int rc = rdv_mlp_spec_check(a.s)) {
      const std::string why = rdv_last_error();
      return fail(rc, "%s: %s: %s", who, a.name, why.c_str());
    }
  return RDV_OK;
}
int rdv_ppo_mlp_spec_check(const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec) {
  return check_spec_pair("rdv_ppo_mlp_spec_check", actor_spec, critic_spec, "actor", "critic");
}

// (a bad spec: the two size queries answer -1; rdv_last_error holds rdv_mlp_spec_check's reason)
static bool mlp_spec_ok(const RdvMlpSpec* spec) { return rdv_mlp_spec_check(spec) == RDV_OK; }

int64_t rdv_ppo_mlp_grad_floats(const RdvMlpSpec* spec, int is_actor) {
  if (!mlp_spec_ok(spec)) return -1;
  PpoMlpTable t;
  ppo_mlp_table(*spec, is_actor != 0, t);
  return t.grad_floats;
}

// the general layout's bytes; a default pair runs the shipped kernels, whose workspace (smaller: the same rows, shorter backward blocks) it covers
static int64_t ppo_mlp_bytes(const RdvMlpSpec& actor_spec, const RdvMlpSpec& critic_spec, int64_t n) {
  PpoMlpTable a, c;
  ppo_mlp_table(actor_spec, true, a);
  ppo_mlp_table(critic_spec, false, c);
  int64_t bytes = ppo_mlp_workspace_floats(a, c, n) * (int64_t)sizeof(float);
  if (is_default_spec(actor_spec) && is_default_spec(critic_spec) && bytes < ppo_workspace_bytes(n)) bytes = ppo_workspace_bytes(n);
  return bytes;
}
int64_t rdv_ppo_mlp_workspace_bytes(const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec, int64_t n) {
  if (n <= 0 || !mlp_spec_ok(actor_spec) || !mlp_spec_ok(critic_spec)) return -1;
  return ppo_mlp_bytes(*actor_spec, *critic_spec, n);
}

// the blocks of two general handles have the sizes of their specs' tables (they were packed from those specs: anything else is a bug)
static int check_block_floats(const char* who, rdv_policy actor, rdv_policy critic, const PpoMlpTable& ta, const PpoMlpTable& tc) {
  if (ta.block_floats != actor->block_floats || tc.block_floats != critic->block_floats)
    return fail(RDV_ERR_HIP, "%s: the handles' blocks have %d and %d floats, their specs say %d and %d", who, actor->block_floats, critic->block_floats, ta.block_floats, tc.block_floats);
  return RDV_OK;
}

int rdv_ppo_mlp_loss_grad(rdv_policy actor, rdv_policy critic, const RdvPpoRows* rows, int64_t n, double clip_range, double ent_coef, double vf_coef,
                          void* workspace, int64_t workspace_bytes, const RdvPpoOut* out, void* stream) {
  const char* who = "rdv_ppo_mlp_loss_grad";
  if (int rc = check_ppo_call(who, rows, out, workspace, false, n, 0, nullptr)) return rc;
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  auto no_set = [&](rdv_policy p, const char* name) -> int {
    return p->n_members > 1 ? fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle is a policy set of %d members: its gradients are not built (the shipped architecture: rdv_ppo_set_loss_grad)", who, name, p->n_members) : RDV_OK;
  };
  if (int rc = check_ppo_handles(who, actor, critic, {false, "actor", "critic", "rdv_critic_create_mlp", "rdv_policy_create_mlp"}, no_set, [] { return RDV_OK; })) return rc;
  if (actor->shipped_arch != critic->shipped_arch)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle has the default spec (the shipped block and kernels), the %s handle another: the mixed pair is not built", who,
                actor->shipped_arch ? "actor" : "critic", actor->shipped_arch ? "critic" : "actor");
  const int64_t need = ppo_mlp_bytes(actor->spec, critic->spec, n);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, n = %lld and these specs need %lld (rdv_ppo_mlp_workspace_bytes)", who, (long long)workspace_bytes, (long long)n, (long long)need);
  // the default pair: the shipped blocks and the kernels of rdv_ppo_loss_grad, its bits
  if (actor->shipped_arch) return rdv_ppo_loss_grad(actor, critic, rows, n, clip_range, ent_coef, vf_coef, workspace, workspace_bytes, out, stream);
  PpoMlpTable ta, tc;
  ppo_mlp_table(actor->spec, true, ta);
  ppo_mlp_table(critic->spec, false, tc);
  if (int rc = check_block_floats(who, actor, critic, ta, tc)) return rc;
  DeviceGuard guard(actor->device);
  if (int rc = raise_ppo_lds_limit(ppo_mlp_raise_lds_limit, g_ppo_mlp_lds_raised, actor->device)) return rc;
  PpoMlpLaunch a = {actor->weights, critic->weights, actor->spec.activation, critic->spec.activation, ta, tc,
                    rows->obs, rows->actions, rows->old_log_prob, rows->advantages, rows->returns, rows->indices, n,
                    ppo_coefs(clip_range, ent_coef, vf_coef), static_cast<float*>(workspace), out->actor_grad, out->critic_grad, out->scalars, out->log_prob, out->values};
  ppo_mlp_launch(a, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- recurrent PPO minibatch gradients (csrc/rdv_ppo_lstm.h): a stand-alone recurrent actor and critic, whole env columns, back through time
int rdv_lstm_ppo_spec_check(const RdvLstmSpec* actor_spec, const RdvLstmSpec* critic_spec) {
  const char* who = "rdv_lstm_ppo_spec_check";
  if (!actor_spec || !critic_spec) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: null %s", who, !actor_spec ? "actor_spec" : "critic_spec");
  const struct { const RdvLstmSpec* s; const char* name; } nets[] = {{actor_spec, "actor"}, {critic_spec, "critic"}};
  for (const auto& a : nets)
    if (int rc = rdv_lstm_spec_check(a.s)) {
      const std::string why = rdv_last_error();
      return fail(rc, "%s: %s: %s", who, a.name, why.c_str());
    }
  if (actor_spec->hidden_size != critic_spec->hidden_size)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the actor's LSTM has %d units, the critic's %d: one hidden_size for both is served", who,
                actor_spec->hidden_size, critic_spec->hidden_size);
  return RDV_OK;
}
int64_t rdv_lstm_ppo_grad_floats(const RdvLstmSpec* spec, int is_actor) {
  if (rdv_lstm_spec_check(spec) != RDV_OK) return -1;
  LstmPpoNet n;
  lstm_ppo_net(spec->hidden_size, spec->trunk, is_actor != 0, n);
  return n.grad_floats;
}
static int64_t lstm_ppo_bytes(int H, const RdvMlpSpec& actor_trunk, const RdvMlpSpec& critic_trunk, int64_t n_steps, int64_t n_seq) {
  LstmPpoNet a, c;
  lstm_ppo_net(H, actor_trunk, true, a);
  lstm_ppo_net(H, critic_trunk, false, c);
  LstmPpoWs w;
  lstm_ppo_workspace(a, c, n_steps, n_seq, w);
  return w.total * (int64_t)sizeof(float);
}
int64_t rdv_lstm_ppo_workspace_bytes(const RdvLstmSpec* actor_spec, const RdvLstmSpec* critic_spec, int64_t n_steps, int64_t n_seq) {
  if (n_steps <= 0 || n_seq <= 0 || rdv_lstm_ppo_spec_check(actor_spec, critic_spec) != RDV_OK) return -1;
  return lstm_ppo_bytes(actor_spec->hidden_size, actor_spec->trunk, critic_spec->trunk, n_steps, n_seq);
}
static bool g_lstm_ppo_lds_raised[64];

int rdv_lstm_ppo_loss_grad(rdv_policy actor, rdv_policy critic, const RdvLstmPpoRows* rows, double clip_range, double ent_coef, double vf_coef,
                           void* workspace, int64_t workspace_bytes, const RdvLstmPpoOut* out, void* stream) {
  const char* who = "rdv_lstm_ppo_loss_grad";
  if (!rows) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows is null", who);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: out is null", who);
  const struct { const void* p; const char* name; } ptrs[] = {
      {rows->obs, "rows->obs"}, {rows->actions, "rows->actions"}, {rows->old_log_prob, "rows->old_log_prob"}, {rows->advantages, "rows->advantages"},
      {rows->returns, "rows->returns"}, {rows->done, "rows->done"}, {rows->actor_h0, "rows->actor_h0"}, {rows->actor_c0, "rows->actor_c0"},
      {rows->critic_h0, "rows->critic_h0"}, {rows->critic_c0, "rows->critic_c0"}, {out->actor_grad, "out->actor_grad"},
      {out->critic_grad, "out->critic_grad"}, {out->scalars, "out->scalars"}, {workspace, "workspace"}};
  for (const auto& a : ptrs) if (!a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is null", who, a.name);
  if (rows->n_envs <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_envs must be positive (got %lld)", who, (long long)rows->n_envs);
  if (rows->n_steps <= 0 || rows->n_steps > (1 << 20))
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_steps must be in 1..2^20 (got %lld)", who, (long long)rows->n_steps);
  if (rows->n_seq <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_seq must be positive (got %lld)", who, (long long)rows->n_seq);
  if (!rows->envs && rows->n_seq > rows->n_envs)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_seq = %lld exceeds rows->n_envs = %lld and rows->envs is null", who, (long long)rows->n_seq, (long long)rows->n_envs);
  if (rows->n_steps * rows->n_seq > (int64_t)1 << 31)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_steps x rows->n_seq = %lld rows: at most 2^31 in one call", who, (long long)(rows->n_steps * rows->n_seq));
  if (misaligned(workspace, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  RDV_CHECK_POLICY(actor);
  RDV_CHECK_POLICY(critic);
  const struct { rdv_policy p; const char* name; } nets[] = {{actor, "actor"}, {critic, "critic"}};
  for (const auto& a : nets) {
    if (!a.p->lstm_hidden)
      return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle is not a recurrent policy (rdv_lstm_policy_create / rdv_lstm_critic_create): rdv_ppo_mlp_loss_grad serves it", who, a.name);
    if (a.p->n_members > 1)
      return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the %s handle is a recurrent set of %d members: its gradients are not built", who, a.name, a.p->n_members);
  }
  if (actor->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor is a critic handle (rdv_lstm_critic_create): actor and critic are swapped", who);
  if (critic->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: critic is an actor handle (rdv_lstm_policy_create): actor and critic are swapped", who);
  if (actor->lstm_hidden != critic->lstm_hidden)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the actor's LSTM has %d units, the critic's %d: one hidden_size for both is served", who, actor->lstm_hidden, critic->lstm_hidden);
  if (actor->device != critic->device) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor on device %d, critic on device %d", who, actor->device, critic->device);
  const int64_t need = lstm_ppo_bytes(actor->lstm_hidden, actor->spec, critic->spec, rows->n_steps, rows->n_seq);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, n_steps = %lld, n_seq = %lld and these specs need %lld (rdv_lstm_ppo_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)rows->n_steps, (long long)rows->n_seq, (long long)need);
  DeviceGuard guard(actor->device);
  if (int rc = raise_ppo_lds_limit(lstm_ppo_raise_lds_limit, g_lstm_ppo_lds_raised, actor->device)) return rc;
  LstmPpoLaunch a = {};
  a.actor_block = actor->weights; a.critic_block = critic->weights;
  a.actor_act = actor->spec.activation; a.critic_act = critic->spec.activation;
  lstm_ppo_net(actor->lstm_hidden, actor->spec, true, a.actor);
  lstm_ppo_net(critic->lstm_hidden, critic->spec, false, a.critic);
  a.obs = rows->obs; a.actions = rows->actions; a.old_log_prob = rows->old_log_prob; a.advantages = rows->advantages; a.returns = rows->returns;
  a.done = rows->done; a.actor_h0 = rows->actor_h0; a.actor_c0 = rows->actor_c0; a.critic_h0 = rows->critic_h0; a.critic_c0 = rows->critic_c0;
  a.envs = rows->envs; a.n_envs = rows->n_envs; a.n_steps = rows->n_steps; a.n_seq = rows->n_seq;
  a.k = ppo_coefs(clip_range, ent_coef, vf_coef);
  a.workspace = static_cast<float*>(workspace);
  a.actor_grad = out->actor_grad; a.critic_grad = out->critic_grad; a.scalars = out->scalars; a.log_prob = out->log_prob; a.values = out->values;
  lstm_ppo_launch(a, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- PPO minibatch gradients for policy sets (csrc/rdv_ppo.h, "the set form")
// 1 .. kPpoSetMaxMembers counts, none negative, one positive
static bool ppo_counts_ok(int32_t n_members, const int64_t* counts_host) {
  if (n_members < 1 || n_members > kPpoSetMaxMembers || !counts_host) return false;
  bool any = false;
  for (int32_t g = 0; g < n_members; ++g) {
    if (counts_host[g] < 0) return false;
    any = any || counts_host[g] > 0;
  }
  return any;
}
static int32_t capped_members(rdv_policy actor_set);
static int check_set_members(const char* who, rdv_policy actor_set, rdv_policy critic_set);

// ---- recurrent PPO minibatch gradients for recurrent sets (csrc/rdv_ppo_lstm.h, "the set form")
int64_t rdv_lstm_ppo_set_workspace_bytes(const RdvLstmSpec* actor_spec, const RdvLstmSpec* critic_spec, int64_t n_steps, int32_t n_members,
                                         const int64_t* counts_host) {
  if (n_steps <= 0 || !ppo_counts_ok(n_members, counts_host) || rdv_lstm_ppo_spec_check(actor_spec, critic_spec) != RDV_OK) return -1;
  // member by member what rdv_lstm_ppo_workspace_bytes answers for one: the sum rule
  int64_t bytes = 0;
  for (int32_t g = 0; g < n_members; ++g)
    if (counts_host[g] > 0) bytes += lstm_ppo_bytes(actor_spec->hidden_size, actor_spec->trunk, critic_spec->trunk, n_steps, counts_host[g]);
  return bytes;
}

int rdv_lstm_ppo_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvLstmPpoRows* rows, const int64_t* counts_host, double clip_range,
                               double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes, const RdvLstmPpoSetOut* out, void* stream) {
  const char* who = "rdv_lstm_ppo_set_loss_grad";
  if (!rows) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows is null", who);
  if (!out) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: out is null", who);
  if (!counts_host) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host is null", who);
  const struct { const void* p; const char* name; } ptrs[] = {
      {rows->obs, "rows->obs"}, {rows->actions, "rows->actions"}, {rows->old_log_prob, "rows->old_log_prob"}, {rows->advantages, "rows->advantages"},
      {rows->returns, "rows->returns"}, {rows->done, "rows->done"}, {rows->actor_h0, "rows->actor_h0"}, {rows->actor_c0, "rows->actor_c0"},
      {rows->critic_h0, "rows->critic_h0"}, {rows->critic_c0, "rows->critic_c0"}, {rows->envs, "rows->envs"}, {out->actor_grad, "out->actor_grad"},
      {out->critic_grad, "out->critic_grad"}, {out->scalars, "out->scalars"}, {workspace, "workspace"}};
  for (const auto& a : ptrs) if (!a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is null", who, a.name);
  const int32_t P = capped_members(actor_set);
  int64_t total = 0, most = 0;
  for (int32_t g = 0; g < P; ++g) {
    if (counts_host[g] < 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host[%d] = %lld is negative", who, g, (long long)counts_host[g]);
    total = counts_host[g] > INT64_MAX - total ? INT64_MAX : total + counts_host[g];
    if (counts_host[g] > most) most = counts_host[g];
  }
  if (total == 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: counts_host holds no positive count (%d member%s)", who, P, P == 1 ? "" : "s");
  if (rows->n_seq != total)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_seq = %lld, counts_host sums to %lld", who, (long long)rows->n_seq, (long long)total);
  if (rows->n_envs <= 0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_envs must be positive (got %lld)", who, (long long)rows->n_envs);
  if (rows->n_steps <= 0 || rows->n_steps > (1 << 20))
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_steps must be in 1..2^20 (got %lld)", who, (long long)rows->n_steps);
  if (most > ((int64_t)1 << 31) / rows->n_steps)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: rows->n_steps = %lld x the largest count %lld: at most 2^31 rows in a member", who, (long long)rows->n_steps, (long long)most);
  if (misaligned(workspace, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  RDV_CHECK_POLICY(actor_set);
  RDV_CHECK_POLICY(critic_set);
  const struct { rdv_policy p; const char* name; } nets[] = {{actor_set, "actor_set"}, {critic_set, "critic_set"}};
  for (const auto& a : nets)
    if (!a.p->lstm_hidden)
      return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is not a recurrent policy or a recurrent set (rdv_lstm_policy_set_create / rdv_lstm_critic_set_create): rdv_ppo_mlp_set_loss_grad serves it", who, a.name);
  if (actor_set->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set is a critic handle (rdv_lstm_critic_set_create): actor and critic are swapped", who);
  if (critic_set->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: critic_set is an actor handle (rdv_lstm_policy_set_create): actor and critic are swapped", who);
  if (int rc = check_set_members(who, actor_set, critic_set)) return rc;
  if (actor_set->lstm_hidden != critic_set->lstm_hidden)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the actors' LSTM has %d units, the critics' %d: one hidden_size for both is served", who, actor_set->lstm_hidden, critic_set->lstm_hidden);
  if (actor_set->device != critic_set->device)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set on device %d, critic_set on device %d", who, actor_set->device, critic_set->device);
  LstmPpoSetLaunch L = {};
  LstmPpoLaunch& a = L.a;
  lstm_ppo_net(actor_set->lstm_hidden, actor_set->spec, true, a.actor);
  lstm_ppo_net(critic_set->lstm_hidden, critic_set->spec, false, a.critic);
  const int64_t need = lstm_ppo_set_table(a.actor, a.critic, rows->n_steps, P, counts_host, &L.table, &L.max_count);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, n_steps = %lld, these counts and specs need %lld (rdv_lstm_ppo_set_workspace_bytes)", who,
                (long long)workspace_bytes, (long long)rows->n_steps, (long long)need);
  DeviceGuard guard(actor_set->device);
  if (int rc = raise_ppo_lds_limit(lstm_ppo_raise_lds_limit, g_lstm_ppo_lds_raised, actor_set->device)) return rc;
  a.actor_block = actor_set->weights; a.critic_block = critic_set->weights;
  a.actor_act = actor_set->spec.activation; a.critic_act = critic_set->spec.activation;
  a.obs = rows->obs; a.actions = rows->actions; a.old_log_prob = rows->old_log_prob; a.advantages = rows->advantages; a.returns = rows->returns;
  a.done = rows->done; a.actor_h0 = rows->actor_h0; a.actor_c0 = rows->actor_c0; a.critic_h0 = rows->critic_h0; a.critic_c0 = rows->critic_c0;
  a.envs = rows->envs; a.n_envs = rows->n_envs; a.n_steps = rows->n_steps; a.n_seq = rows->n_seq;
  a.k = ppo_coefs(clip_range, ent_coef, vf_coef);
  a.workspace = static_cast<float*>(workspace);
  a.actor_grad = out->actor_grad; a.critic_grad = out->critic_grad; a.scalars = out->scalars; a.log_prob = out->log_prob; a.values = out->values;
  L.n_members = P; L.actor_block_floats = actor_set->block_floats; L.critic_block_floats = critic_set->block_floats;
  lstm_ppo_set_launch(L, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}
int64_t rdv_ppo_set_workspace_bytes(int32_t n_members, const int64_t* counts_host) {
  return ppo_counts_ok(n_members, counts_host) ? ppo_set_table(n_members, counts_host, nullptr) : -1;
}

// The member count that the host-only checks of a set entry point judge counts_host or the mask by: one entry or bit per member of the
// handles.  With an invalid actor handle (refused behind those checks) it is one member's; a set larger than the cap (refused behind them
// too, before anything past the cap is looked at) counts as the cap's.
static int32_t capped_members(rdv_policy actor_set) {
  const bool valid = actor_set && actor_set->magic == kPolicyMagic;
  return valid ? (actor_set->n_members < kPpoSetMaxMembers ? actor_set->n_members : kPpoSetMaxMembers) : 1;
}

// different member counts, more members than one call serves: every set entry point's last two refusals of the architecture
static int check_set_members(const char* who, rdv_policy actor_set, rdv_policy critic_set) {
  if (actor_set->n_members != critic_set->n_members)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set has %d members, critic_set has %d", who, actor_set->n_members, critic_set->n_members);
  if (actor_set->n_members > kPpoSetMaxMembers)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set has %d members, at most %d are served by one call (kPpoSetMaxMembers)", who, actor_set->n_members, kPpoSetMaxMembers);
  return RDV_OK;
}
// what the set entry points (rdv_ppo_set_loss_grad, rdv_ppo_set_adam_step) refuse of the architecture of two valid feed-forward sets, in this
// order: another architecture than the shipped one, different member counts, more members than one call serves
static int check_shipped_sets(const char* who, rdv_policy actor_set, rdv_policy critic_set, const char* not_built) {
  const struct { rdv_policy p; const char* name; } nets[] = {{actor_set, "actor_set"}, {critic_set, "critic_set"}};
  for (const auto& a : nets)
    if (!is_default_spec(a.p->spec) || !a.p->shipped_arch)
      return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is not the shipped architecture (two hidden layers of 64, tanh): %s", who, a.name, not_built);
  return check_set_members(who, actor_set, critic_set);
}

int rdv_ppo_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvPpoRows* rows, const int64_t* counts_host, double clip_range,
                          double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes, const RdvPpoSetOut* out, void* stream) {
  const char* who = "rdv_ppo_set_loss_grad";
  const int32_t P = capped_members(actor_set);
  if (int rc = check_ppo_call(who, rows, out, workspace, true, 0, P, counts_host)) return rc;
  PpoSetLaunch L = {};
  const int64_t need = ppo_set_table(P, counts_host, &L.table, nullptr, &L.max_workgroups);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, these counts need %lld (rdv_ppo_set_workspace_bytes)", who, (long long)workspace_bytes, (long long)need);
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  auto shipped_sets = [&]() -> int { return check_shipped_sets(who, actor_set, critic_set, "its gradients are not built"); };
  if (int rc = check_ppo_handles(who, actor_set, critic_set, {true, "actor_set", "critic_set", "rdv_critic_set_create", "rdv_policy_set_create"},
                                 [](rdv_policy, const char*) { return RDV_OK; }, shipped_sets)) return rc;
  DeviceGuard guard(actor_set->device);
  if (int rc = raise_ppo_lds_limit(ppo_raise_lds_limit, g_ppo_lds_raised, actor_set->device)) return rc;
  L.a = {actor_set->weights, critic_set->weights, rows->obs, rows->actions, rows->old_log_prob, rows->advantages, rows->returns, rows->indices, 0,
         ppo_coefs(clip_range, ent_coef, vf_coef), static_cast<float*>(workspace), out->actor_grad, out->critic_grad, out->scalars, out->log_prob, out->values};
  L.n_members = P;
  ppo_set_launch(L, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- PPO minibatch gradients for policy sets of every MLP architecture (csrc/rdv_ppo_mlp.h, "the set form")
int rdv_ppo_mlp_set_spec_check(const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec) {
  if (int rc = check_spec_pair("rdv_ppo_mlp_set_spec_check", actor_spec, critic_spec, "actor_set", "critic_set")) return rc;
  // (is_shipped: the predicate that gives a handle its shipped block and kernels, i.e. what check_mlp_sets reads off the handles)
  if (is_shipped(actor_spec) != is_shipped(critic_spec))
    return fail(RDV_ERR_INVALID_ARGUMENT, "rdv_ppo_mlp_set_loss_grad, rdv_ppo_mlp_set_adam_step: %s has the default spec (the shipped block and kernels), %s another: the mixed pair is not built",
                is_shipped(actor_spec) ? "actor_set" : "critic_set", is_shipped(actor_spec) ? "critic_set" : "actor_set");
  return RDV_OK;
}

// the general layout's table and bytes for a pair of general specs
static int64_t ppo_mlp_set_bytes(const RdvMlpSpec& actor_spec, const RdvMlpSpec& critic_spec, int32_t n_members, const int64_t* counts, PpoMlpSetLaunch* L) {
  PpoMlpTable a, c;
  ppo_mlp_table(actor_spec, true, a);
  ppo_mlp_table(critic_spec, false, c);
  if (L) { L->a.actor = a; L->a.critic = c; }
  return ppo_mlp_set_table(a, c, n_members, counts, L ? &L->table : nullptr, L ? &L->max_groups_a : nullptr, L ? &L->max_groups_c : nullptr);
}
int64_t rdv_ppo_mlp_set_workspace_bytes(const RdvMlpSpec* actor_spec, const RdvMlpSpec* critic_spec, int32_t n_members, const int64_t* counts_host) {
  if (!mlp_spec_ok(actor_spec) || !mlp_spec_ok(critic_spec) || !ppo_counts_ok(n_members, counts_host)) return -1;
  // member by member what rdv_ppo_mlp_workspace_bytes answers for one (for the default pair the larger of the two layouts): the sum rule
  int64_t bytes = 0;
  for (int32_t g = 0; g < n_members; ++g)
    if (counts_host[g] > 0) bytes += ppo_mlp_bytes(*actor_spec, *critic_spec, counts_host[g]);
  return bytes;
}

// both handles valid feed-forward sets (or plain handles) of the default spec on the shipped kernels: the set calls of rdv_ppo.h / rdv_ppo_adam.h serve them
static bool shipped_pair(rdv_policy a, rdv_policy c) {
  const auto ok = [](rdv_policy p) { return p && p->magic == kPolicyMagic && !p->lstm_hidden && p->shipped_arch && is_default_spec(p->spec); };
  return ok(a) && ok(c);
}
// what the two general set entry points refuse of the architecture of two valid feed-forward sets: the mixed pair, then check_set_members
static int check_mlp_sets(const char* who, rdv_policy actor_set, rdv_policy critic_set) {
  if (actor_set->shipped_arch != critic_set->shipped_arch)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s has the default spec (the shipped block and kernels), %s another: the mixed pair is not built", who,
                actor_set->shipped_arch ? "actor_set" : "critic_set", actor_set->shipped_arch ? "critic_set" : "actor_set");
  return check_set_members(who, actor_set, critic_set);
}

int rdv_ppo_mlp_set_loss_grad(rdv_policy actor_set, rdv_policy critic_set, const RdvPpoRows* rows, const int64_t* counts_host, double clip_range,
                              double ent_coef, double vf_coef, void* workspace, int64_t workspace_bytes, const RdvPpoSetOut* out, void* stream) {
  const char* who = "rdv_ppo_mlp_set_loss_grad";
  // two sets of the default spec: the call IS rdv_ppo_set_loss_grad, its bits and its refusals
  if (shipped_pair(actor_set, critic_set))
    return rdv_ppo_set_loss_grad(actor_set, critic_set, rows, counts_host, clip_range, ent_coef, vf_coef, workspace, workspace_bytes, out, stream);
  const int32_t P = capped_members(actor_set);
  if (int rc = check_ppo_call(who, rows, out, workspace, true, 0, P, counts_host)) return rc;
  if (int rc = check_ppo_coefficients(who, clip_range, ent_coef, vf_coef)) return rc;
  auto sets = [&]() -> int { return check_mlp_sets(who, actor_set, critic_set); };
  if (int rc = check_ppo_handles(who, actor_set, critic_set, {true, "actor_set", "critic_set", "rdv_critic_set_create", "rdv_policy_set_create"},
                                 [](rdv_policy, const char*) { return RDV_OK; }, sets)) return rc;
  PpoMlpSetLaunch L = {};
  const int64_t need = ppo_mlp_set_bytes(actor_set->spec, critic_set->spec, P, counts_host, &L);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, these counts and specs need %lld (rdv_ppo_mlp_set_workspace_bytes)", who, (long long)workspace_bytes, (long long)need);
  const PpoMlpTable ta = L.a.actor, tc = L.a.critic;
  if (int rc = check_block_floats(who, actor_set, critic_set, ta, tc)) return rc;
  DeviceGuard guard(actor_set->device);
  if (int rc = raise_ppo_lds_limit(ppo_mlp_raise_lds_limit, g_ppo_mlp_lds_raised, actor_set->device)) return rc;
  L.a = {actor_set->weights, critic_set->weights, actor_set->spec.activation, critic_set->spec.activation, ta, tc,
         rows->obs, rows->actions, rows->old_log_prob, rows->advantages, rows->returns, rows->indices, 0,
         ppo_coefs(clip_range, ent_coef, vf_coef), static_cast<float*>(workspace), out->actor_grad, out->critic_grad, out->scalars, out->log_prob, out->values};
  L.n_members = P;
  ppo_mlp_set_launch(L, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- gradient clip, Adam and weight repack for policy sets (csrc/rdv_ppo_adam.h)
extern "C++" {
// The host-only checks of the two optimiser entry points, in this order: state and every pointer non-null, 16-byte aligned; the five
// scalars; the mask, against P = capped_members(actor_set).
static int check_adam_call(const char* who, rdv_policy actor_set, const RdvAdamState* state, const float* actor_grad, const float* critic_grad,
                           uint64_t active_mask, double lr, double beta1, double beta2, double eps, double max_grad_norm, int32_t& P) {
  if (!state) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: state is null", who);
  const struct { const void* p; const char* name; } ptrs[] = {
      {state->actor_param, "state->actor_param"}, {state->critic_param, "state->critic_param"}, {state->actor_m, "state->actor_m"},
      {state->actor_v, "state->actor_v"}, {state->critic_m, "state->critic_m"}, {state->critic_v, "state->critic_v"}, {state->step, "state->step"},
      {state->coef, "state->coef"}, {actor_grad, "actor_grad"}, {critic_grad, "critic_grad"}};
  for (const auto& a : ptrs) if (!a.p) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is null", who, a.name);
  for (const auto& a : ptrs) if (misaligned(a.p, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s must be 16-byte aligned", who, a.name);
  if (!std::isfinite(lr) || lr <= 0.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: lr must be finite and positive (got %g)", who, lr);
  if (!std::isfinite(eps) || eps <= 0.0) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: eps must be finite and positive (got %g)", who, eps);
  if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: beta1 must be in [0, 1) (got %g)", who, beta1);
  if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: beta2 must be in [0, 1) (got %g)", who, beta2);
  if (!(max_grad_norm > 0.0)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: max_grad_norm must be positive, +inf for no clipping (got %g)", who, max_grad_norm);
  if (!active_mask) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: active_mask is empty: no member takes the step", who);
  P = capped_members(actor_set);
  if (P < 64 && (active_mask >> P)) {
    int bit = 63;
    while (!((active_mask >> bit) & 1)) --bit;
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: active_mask has bit %d set, the set has %d member%s", who, bit, P, P == 1 ? "" : "s");
  }
  return RDV_OK;
}
// the launch of either entry point: the handles' blocks, the caller's arrays with rows of ga / gc floats, the mask and the scalars
static PpoAdamLaunch adam_launch_args(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state, const float* actor_grad, const float* critic_grad,
                                      uint64_t active_mask, int32_t P, int32_t ga, int32_t gc, double lr, double beta1, double beta2, double eps, double max_grad_norm) {
  PpoAdamLaunch a = {};
  a.actor_block = actor_set->weights; a.critic_block = critic_set->weights;
  a.actor_param = state->actor_param; a.critic_param = state->critic_param;
  a.actor_m = state->actor_m; a.actor_v = state->actor_v; a.critic_m = state->critic_m; a.critic_v = state->critic_v;
  a.step = state->step; a.coef = state->coef; a.actor_grad = actor_grad; a.critic_grad = critic_grad;
  a.mask = active_mask; a.n_members = P; a.ga = ga; a.gc = gc;
  return ppo_adam_scalars(a, lr, beta1, beta2, eps, max_grad_norm);
}
}  // extern "C++"

int rdv_ppo_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state, const float* actor_grad, const float* critic_grad,
                          uint64_t active_mask, double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream) {
  const char* who = "rdv_ppo_set_adam_step";
  int32_t P;
  if (int rc = check_adam_call(who, actor_set, state, actor_grad, critic_grad, active_mask, lr, beta1, beta2, eps, max_grad_norm, P)) return rc;
  const char* not_built = "its optimiser step is not built";
  auto shipped_sets = [&]() -> int { return check_shipped_sets(who, actor_set, critic_set, not_built); };
  if (int rc = check_ppo_handles(who, actor_set, critic_set, {true, "actor_set", "critic_set", "rdv_critic_set_create", "rdv_policy_set_create", not_built},
                                 [](rdv_policy, const char*) { return RDV_OK; }, shipped_sets)) return rc;
  if (actor_set->block_floats != kPolFloats || critic_set->block_floats != kPolFloats)
    return fail(RDV_ERR_HIP, "%s: the handles' blocks have %d and %d floats, the shipped block %d", who, actor_set->block_floats, critic_set->block_floats, kPolFloats);
  DeviceGuard guard(actor_set->device);
  ppo_adam_launch(adam_launch_args(actor_set, critic_set, state, actor_grad, critic_grad, active_mask, P, kPpoActorGrad, kPpoCriticGrad, lr, beta1, beta2, eps, max_grad_norm),
                  static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- gradient clip, Adam and weight repack for policy sets of every MLP architecture (csrc/rdv_ppo_adam.h, "every MLP architecture")
int rdv_ppo_mlp_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state, const float* actor_grad, const float* critic_grad,
                              uint64_t active_mask, double lr, double beta1, double beta2, double eps, double max_grad_norm, void* stream) {
  const char* who = "rdv_ppo_mlp_set_adam_step";
  // two sets of the default spec: the call IS rdv_ppo_set_adam_step, its bits and its refusals
  if (shipped_pair(actor_set, critic_set))
    return rdv_ppo_set_adam_step(actor_set, critic_set, state, actor_grad, critic_grad, active_mask, lr, beta1, beta2, eps, max_grad_norm, stream);
  int32_t P;
  if (int rc = check_adam_call(who, actor_set, state, actor_grad, critic_grad, active_mask, lr, beta1, beta2, eps, max_grad_norm, P)) return rc;
  const char* not_built = "its optimiser step is not built";
  auto sets = [&]() -> int { return check_mlp_sets(who, actor_set, critic_set); };
  if (int rc = check_ppo_handles(who, actor_set, critic_set, {true, "actor_set", "critic_set", "rdv_critic_set_create", "rdv_policy_set_create", not_built},
                                 [](rdv_policy, const char*) { return RDV_OK; }, sets)) return rc;
  PpoMlpAdamLaunch A = {};
  ppo_mlp_table(actor_set->spec, true, A.T[0]);
  ppo_mlp_table(critic_set->spec, false, A.T[1]);
  if (int rc = check_block_floats(who, actor_set, critic_set, A.T[0], A.T[1])) return rc;
  DeviceGuard guard(actor_set->device);
  A.a = adam_launch_args(actor_set, critic_set, state, actor_grad, critic_grad, active_mask, P, A.T[0].grad_floats, A.T[1].grad_floats, lr, beta1, beta2, eps, max_grad_norm);
  ppo_mlp_adam_launch(A, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

// ---- gradient clip, Adam and weight repack for recurrent policy sets (csrc/rdv_ppo_lstm_adam.h)
int64_t rdv_lstm_ppo_adam_workspace_bytes(const RdvLstmSpec* actor_spec, const RdvLstmSpec* critic_spec, int32_t n_members) {
  if (n_members < 1 || n_members > kPpoSetMaxMembers || rdv_lstm_ppo_spec_check(actor_spec, critic_spec) != RDV_OK) return -1;
  LstmAdamLaunch L = {};
  lstm_adam_net(actor_spec->hidden_size, actor_spec->trunk, true, L.net[0]);
  lstm_adam_net(critic_spec->hidden_size, critic_spec->trunk, false, L.net[1]);
  return lstm_adam_workspace(L, n_members);
}

int rdv_lstm_ppo_set_adam_step(rdv_policy actor_set, rdv_policy critic_set, const RdvAdamState* state, const float* actor_grad, const float* critic_grad,
                               uint64_t active_mask, double lr, double beta1, double beta2, double eps, double max_grad_norm, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  const char* who = "rdv_lstm_ppo_set_adam_step";
  int32_t P;
  if (int rc = check_adam_call(who, actor_set, state, actor_grad, critic_grad, active_mask, lr, beta1, beta2, eps, max_grad_norm, P)) return rc;
  if (!workspace) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace is null", who);
  if (misaligned(workspace, 16)) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  RDV_CHECK_POLICY(actor_set);
  RDV_CHECK_POLICY(critic_set);
  const struct { rdv_policy p; const char* name; } nets[] = {{actor_set, "actor_set"}, {critic_set, "critic_set"}};
  for (const auto& a : nets)
    if (!a.p->lstm_hidden)
      return fail(RDV_ERR_INVALID_ARGUMENT, "%s: %s is not a recurrent policy or a recurrent set (rdv_lstm_policy_set_create / rdv_lstm_critic_set_create): rdv_ppo_mlp_set_adam_step serves it", who, a.name);
  if (actor_set->out_dim != kPolOut) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set is a critic handle (rdv_lstm_critic_set_create): actor and critic are swapped", who);
  if (critic_set->out_dim != 1) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: critic_set is an actor handle (rdv_lstm_policy_set_create): actor and critic are swapped", who);
  if (int rc = check_set_members(who, actor_set, critic_set)) return rc;
  if (actor_set->lstm_hidden != critic_set->lstm_hidden)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: the actors' LSTM has %d units, the critics' %d: one hidden_size for both is served", who, actor_set->lstm_hidden, critic_set->lstm_hidden);
  if (actor_set->device != critic_set->device)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: actor_set on device %d, critic_set on device %d", who, actor_set->device, critic_set->device);
  LstmAdamLaunch L = {};
  lstm_adam_net(actor_set->lstm_hidden, actor_set->spec, true, L.net[0]);
  lstm_adam_net(critic_set->lstm_hidden, critic_set->spec, false, L.net[1]);
  const int64_t need = lstm_adam_workspace(L, P);
  if (workspace_bytes < need)
    return fail(RDV_ERR_INVALID_ARGUMENT, "%s: workspace_bytes = %lld, %d member%s of these specs need %lld (rdv_lstm_ppo_adam_workspace_bytes)", who,
                (long long)workspace_bytes, P, P == 1 ? "" : "s", (long long)need);
  if (L.net[0].block_floats != actor_set->block_floats || L.net[1].block_floats != critic_set->block_floats)
    return fail(RDV_ERR_HIP, "%s: the handles' blocks have %d and %d floats, their specs say %d and %d", who, actor_set->block_floats, critic_set->block_floats,
                L.net[0].block_floats, L.net[1].block_floats);
  DeviceGuard guard(actor_set->device);
  L.a = adam_launch_args(actor_set, critic_set, state, actor_grad, critic_grad, active_mask, P, L.net[0].grad_floats, L.net[1].grad_floats, lr, beta1, beta2, eps, max_grad_norm);
  L.ws = static_cast<char*>(workspace);
  lstm_adam_launch(L, static_cast<hipStream_t>(stream));
  RDV_HIP(hipGetLastError());
  return RDV_OK;
}

int64_t rdv_policy_block_floats(rdv_policy p) { return (p && p->magic == kPolicyMagic) ? p->block_floats : -1; }

int rdv_policy_get_block(rdv_policy p, int32_t member, float* out_host, int64_t floats, void* stream) {
  const char* who = "rdv_policy_get_block";
  RDV_CHECK_POLICY(p);
  if (!out_host) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: out_host is null", who);
  if (member < 0 || member >= p->n_members) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: member %d of %d", who, member, p->n_members);
  if (floats != p->block_floats) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: floats = %lld, the handle's block has %d (rdv_policy_block_floats)", who, (long long)floats, p->block_floats);
  DeviceGuard guard(p->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = refuse_in_capture(who, s)) return rc;
  RDV_HIP(hipMemcpyAsync(out_host, p->weights + (size_t)p->block_floats * (size_t)member, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost, s));
  RDV_HIP(hipStreamSynchronize(s));
  return RDV_OK;
}

}  // extern "C"

// rdv_host.h — what the two host units of the C ABI share: rdv_hip.hip (env handles, and rdv_rollout, which reads a policy handle) and
// rdv_policy_host.hip (policy handles).  HOST CODE ONLY: no __device__ function, no kernel, nothing the device compiler emits, so
// including it leaves every kernel's instructions what they were.  The functions declared (not defined) here are internal to the
// library: hidden, so the set of exported symbols is include/rdv.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/rdv.h"

#define RDV_INTERNAL __attribute__((visibility("hidden")))

namespace rdv {

// the message behind rdv_last_error (one thread_local buffer, in rdv_hip.hip); returns `code`
RDV_INTERNAL int fail(int code, const char* fmt, ...);
// A failed HIP call also leaves its code in the runtime's per-thread "last error", which the NEXT caller of hipGetLastError() would
// be handed — e.g. PyTorch's launch check after its next kernel, which would then raise for a failure that was ours and has been
// reported through this ABI.  Reading it here clears it.
#define RDV_HIP(call)                                                                                       \
  do {                                                                                                      \
    hipError_t err__ = (call);                                                                              \
    if (err__ != hipSuccess) {                                                                              \
      (void)hipGetLastError();                                                                              \
      return fail(err__ == hipErrorOutOfMemory ? RDV_ERR_OUT_OF_MEMORY : RDV_ERR_HIP,                       \
                  "%s failed: %s", #call, hipGetErrorString(err__));                                        \
    }                                                                                                       \
  } while (0)

static inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
static inline bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
// THE tile table of parameter groups and policy sets (group g of n owns the next sizes[g] rows): tile t -> the owner of row t * tile; past the last tile: n - 1
static inline std::vector<int32_t> tile_table(const int64_t* sizes, int32_t n, int64_t tile, int64_t entries) {
  std::vector<int32_t> table((size_t)entries, n - 1);
  for (int64_t g = 0, at = 0; g < n; at += sizes[g++])
    for (int64_t t = at / tile; t < (at + sizes[g] + tile - 1) / tile && t < entries; ++t) table[(size_t)t] = (int32_t)g;
  return table;
}

struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
// `device` exists: checked by every call that creates a handle (`who`, for the message)
static inline int check_device(const char* who, int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(RDV_ERR_NO_DEVICE, "no HIP device available: this library has no CPU path");
  if (device < 0 || device >= count) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: device %d out of range [0,%d)", who, device, count);
  return RDV_OK;
}
// The calls that synchronise `s` or allocate (rdv_get_stats, rdv_get_group_stats, rdv_eval_summary, rdv_eval_group_summary, rdv_restore,
// rdv_set_param_groups) are not legal while `s` records a graph: the runtime would fail the call and invalidate the capture.  They ask
// here before they touch the stream, and refuse with the capture intact (include/rdv.h, "Stream capture").  `why`: the reason the
// message gives (the weight refresh of rdv_policy_host.hip has one of its own).
static inline int refuse_in_capture(const char* who, hipStream_t s, const char* why = "(it synchronises the stream or allocates): call it outside the capture") {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  RDV_HIP(hipStreamIsCapturing(s, &capturing));
  if (capturing != hipStreamCaptureStatusNone) return fail(RDV_ERR_INVALID_ARGUMENT, "%s: not legal inside a stream capture %s", who, why);
  return RDV_OK;
}

}  // namespace rdv

// A policy handle: the shipped actor / critic (csrc/rdv_policy.h), another architecture (csrc/rdv_policy_mlp.h), a policy set
// (csrc/rdv_policy_sets.h) or a recurrent policy (csrc/rdv_policy_lstm.h).  Made and freed by rdv_policy_host.hip alone.
static constexpr uint32_t kPolicyMagic = 0x52445650u;   // "RDVP"
struct RdvPolicyNet {
  uint32_t magic = kPolicyMagic;   // 0 once destroyed
  int device = 0;
  float* weights = nullptr;   // device, kPolFloats floats: the parameter block of csrc/rdv_policy.h (shipped_arch) or block_floats of csrc/rdv_policy_mlp.h
  int out_dim = 0;            // 6: the actor (rdv_policy_create), 1: the critic (rdv_critic_create)
  RdvMlpSpec spec = {};
  bool shipped_arch = false;  // 17-64-64-out tanh: policy_act_kernel / policy_value_kernel, and the persistent rollout_kernel
  int block_floats = 0;
  float* staging = nullptr;   // rdv_policy_set_weights / rdv_policy_set_member_weights: pinned host copies of the blocks in flight, one slot per
                              // member (made by the first call, nullptr before)
  std::vector<hipEvent_t> staged;   // ... per member, recorded behind the copy out of its slot: the next refresh of THAT member waits for it
  // policy sets (csrc/rdv_policy_sets.h): `weights` holds n_members blocks of block_floats floats, then the tile table
  int32_t n_members = 1;      // 1: a plain handle, or a set of one member (the plain kernels read its one block)
  int64_t rows = 0;           // 0: a plain handle (any n); a set: the rows its members own together
  const int32_t* tile_member = nullptr;   // device: member index per 256-row tile (inside the allocation of `weights`); nullptr for a plain handle
  // the recurrent policy (csrc/rdv_policy_lstm.h): lstm_hidden != 0, `weights` = [trunk block | cell block] (a recurrent set: n_members
  // such blocks, then the tile table, as a policy set), `rows` = the rows whose state the handle owns; one device allocation
  // `lstm_state` holds h, c, h_next, c_tmp ([rows, H] fp32 each), obs_tmp [rows, 17], pending [rows]
  int32_t lstm_hidden = 0;
  float *lstm_state = nullptr, *lstm_h = nullptr, *lstm_c = nullptr, *lstm_h_next = nullptr, *lstm_c_tmp = nullptr, *lstm_obs_tmp = nullptr;
  uint8_t* lstm_pending = nullptr;
};
#define RDV_CHECK_POLICY(p) if (!(p) || (p)->magic != kPolicyMagic) return rdv::fail(RDV_ERR_BAD_HANDLE, "invalid rdv_policy")

namespace rdv {
// The act step of rdv_rollout's act + step loop (rdv_policy_host.hip): actor `p` on the n rows `obs` of step t — the set, general MLP,
// shipped or recurrent kernels, as the handle asks.  `done`: the loop's [T][n] done rows; a recurrent actor starts step 0 from its pending
// flags and step t from row t - 1.  The caller's DeviceGuard holds the device; the arguments have been checked.
RDV_INTERNAL int policy_act_step(rdv_policy p, int32_t t, const float* obs, const uint8_t* done, float* actions, int64_t n, int deterministic,
                                 uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s);
}  // namespace rdv

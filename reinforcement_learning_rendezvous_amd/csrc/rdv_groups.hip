// rdv_groups.hip — the kernels of parameter groups (rdv_set_param_groups, include/rdv.h): one batch, G contiguous groups of envs, each
// with its own DevParams block, ONE launch.  The parameter block is wave-uniform by design (every field a scalar load) and a workgroup
// owns 256 consecutive envs in every step layout, so groups that begin on 256-env boundaries cost one more scalar load per workgroup:
// the group index of the workgroup's tile, read from a table in device memory with the LOGICAL block index (behind the XCD reorder),
// and then P = Pp[group] instead of P = *Pp.  A group may not begin inside a tile because the reset-by-part phase shares one block
// among the four waves of a workgroup (refill_pass_lds).
// Its own translation unit so that the objects of rdv_hip.hip stay what they were: the bodies below are those of step_kernel_parts
// (rdv_step.h) and step_kernel (rdv_fused.h) with that one difference — same functions on the same inputs, so an env's results are
// bit for bit those of a stand-alone handle created with its group's parameters (tests/test_gpu_param_groups.py).
#include "rdv_kernels.h"
#include "rdv_slots.h"
#define RDV_COLD_LANES_ONLY
#include "rdv_cold.h"
#include "rdv_groups.h"

namespace rdv {

// The group of a workgroup's tile.  `lblock` is computed from blockIdx and a kernel argument, so the index, the table entry and
// with them the address of every parameter field are wave-uniform: the table entry is ONE scalar load, requested at kernel entry (it
// needs nothing but the block index) and waited for where the first parameter is used, behind the requests of the state.
__device__ __forceinline__ const DevParams& group_block(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, int64_t lblock) {
  const int g = __builtin_amdgcn_readfirstlane(tile_group[lblock]);
  return Pp[g];
}

// ---------------------------------------------------------------------------------------------------------------
// step_kernel_parts (rdv_step.h) for parameter groups: see there for the layout, the staggered start and the reset by part.
template <typename ST, bool kAll>   // kAll: on_done != HALT — every lane runs the transition (advance_all)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(sizeof(ST) == 4 ? RDV_PARTS_WAVES : 3))) void step_kernel_groups(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                             uint64_t* stats_hot, float* obs_hot, float* reward_hot, const int32_t* __restrict__ tile_group, const StepArgs A_rest) {
  const StepArgs A = hot_args(A_rest, ws_hot, actions_hot, n_hot, stats_hot, obs_hot, reward_hot);
  using V = typename Vec4<ST>::type;
  __shared__ __attribute__((aligned(16))) float lds[kBlock * RDV_OBS_DIM];   // observation rows [256][17]
  __shared__ uint32_t job_kind[kBlock];
  __shared__ uint32_t job_counter[kBlock];
  __shared__ uint16_t lists[kGroupWaves * kBlock];
  static_assert(kBlock == kGroupEnvs && kBlock == kGroupTile, "one workgroup = one tile of the group table = one reset-by-part pass");
  const int lane = threadIdx.x & (kWave - 1);
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t lblock = A.xcd_per ? (int64_t)(blockIdx.x & 7) * A.xcd_per + (blockIdx.x >> 3) : (int64_t)blockIdx.x;
  const DevParams& P = group_block(Pp, tile_group, lblock);   // the LOGICAL block: the table is in env order
  const int64_t block_base = lblock * kBlock;
  const int64_t wave_base = block_base + wave_in_block * kWave;
  const int64_t n = A.n;
  const int64_t rows = (n - wave_base) < kWave ? (n - wave_base) : kWave;    // valid envs of this wave (may be <= 0)
  const bool active = lane < rows;
  float* wl = lds + wave_in_block * (kWave * RDV_OBS_DIM);
  V* ws = reinterpret_cast<V*>(A.ws);
  const bool resets = A.on_done == RDV_ON_DONE_RESET;   // kernel-uniform: the barriers below are executed by all waves or by none
  RDV_STAMP_DECL
  RDV_STAMP(0);
  if (A.stagger && blockIdx.x < 1024u) {
    const int slot = (int)(blockIdx.x >> 8);
    for (int k = 0; k < slot * A.stagger; ++k) __builtin_amdgcn_s_sleep(8);
  }

  {
    V* wsw = ws + wave_base;
    const StepArgs Aw = wave_outputs(A, wave_base);
    Env e;
    uint64_t* slot = A.stats + (uint64_t)(wave_base / kWave) * kStatWords;
    uint64_t slot_pre;
    float a[RDV_ACT_DIM];
    constexpr bool kPinned = kAll && sizeof(ST) == 4;
    PinnedInputs pin;
    if constexpr (kPinned) {
      pinned_state(A, wave_base, lane, pin, e);
    } else if constexpr (kAll) {
      TileInputs<ST> in;
      tile_fetch<ST>(A, wave_base, lane, in);
      unpack_env<ST>(in.c, e);
      slot_pre = in.slot_pre;
#pragma unroll
      for (int k = 0; k < 3; ++k) { a[2 * k] = in.a[k].x; a[2 * k + 1] = in.a[k].y; }
    } else {
      if (active) load_env<ST>(wsw, A.cs, lane, e);
      slot_pre = rows > 0 ? stats_preload(slot, lane) : 0ull;
      load_actions(A.actions + wave_base * RDV_ACT_DIM, 0, lane, active, a);
    }
    RDV_STAMP_STATE(e);
    RDV_STAMP(1);
    StepResult r;
    const RowSink my_row{wl + lane * RDV_OBS_DIM};
    constexpr bool kPack = sizeof(ST) == 4;
    V packed[kChunks];
    bool stepped;
    auto actions_ready = [&](double& after) { if constexpr (kPinned) pinned_rest(pin, after, a, slot_pre); };
    if constexpr (kAll) { advance_all<ST>(P, e, a, r, my_row, kPack ? packed : nullptr, actions_ready); stepped = active; }
    else stepped = advance<ST, false, false, false>(A, P, wave_base + lane, active, e, a, r, my_row, NoHook(), kPack ? packed : nullptr);
    RDV_STAMP(2);
    const bool fin = stepped && r.done;
    stats_update(slot, slot_pre, lane, stepped, fin, r.reason, e.flags, e.k, e.ep_ret, e.sum_dv, e.sum_dw);
    store_step_outputs<true>(Aw, lane, active, fin, r, e, my_row.row);
    const bool to_reset = fin && resets;
    halt_if_done<ST>(A, fin, e, kPack ? packed : nullptr);
    if (resets) {
      job_kind[threadIdx.x] = to_reset ? JOB_REFILL : JOB_NONE;
      job_counter[threadIdx.x] = e.episode;
    }
    if (stepped && !to_reset) { if (kPack) store_chunks<ST>(wsw, A.cs, lane, packed, false); else store_env<ST>(wsw, A.cs, lane, e, false); }
  }
  RDV_STAMP(3);
  if (resets) {
    __syncthreads();
    RDV_STAMP(4);
    LiveStore<ST> L;
    L.ws = ws; L.rows = lds; L.cs = A.cs; L.base = block_base;
    refill_pass_lds<ST>(wave_in_block, lane, P, L, job_kind, job_counter, lists + wave_in_block * kBlock, block_base, n, A.seed,
                        A.env_id_offset, A.tape, A.tape_depth);   // the four waves share P: a group begins on a tile boundary
    RDV_STAMP(5);
    __syncthreads();
  } else {
    wave_lds_fence();
  }
  RDV_STAMP(6);
  if (A.stream_rows) store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);
  else store_obs_rows<false>(A.obs, wave_base, rows, lane, wl);
  RDV_STAMP(7);
  RDV_STAMP_FLUSH((uint64_t)blockIdx.x * (kBlock / kWave) + wave_in_block)
}

// ---------------------------------------------------------------------------------------------------------------
// step_kernel (rdv_fused.h) for parameter groups: the evaluator build (kDiag) and the first step after rdv_set_state (kRaw).
template <typename ST, bool kDiag, bool kRaw>
__global__ __launch_bounds__(kBlock) void step_kernel_groups_lane(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                                  uint64_t* stats_hot, float* obs_hot, float* reward_hot, const int32_t* __restrict__ tile_group, const StepArgs A_rest) {
  const StepArgs A = hot_args(A_rest, ws_hot, actions_hot, n_hot, stats_hot, obs_hot, reward_hot);
  using V = typename Vec4<ST>::type;
  __shared__ __attribute__((aligned(16))) float lds[kBlock * RDV_OBS_DIM];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave_in_block = threadIdx.x >> 6;
  const int64_t lblock = A.xcd_per ? (int64_t)(blockIdx.x & 7) * A.xcd_per + (blockIdx.x >> 3) : (int64_t)blockIdx.x;
  const DevParams& P = group_block(Pp, tile_group, lblock);
  const int64_t i = lblock * kBlock + threadIdx.x;
  const int64_t wave_base = i - lane;
  const int64_t n = A.n;
  const bool active = i < n;
  const int64_t rows = (n - wave_base) < kWave ? (n - wave_base) : kWave;
  float* wl = lds + wave_in_block * (kWave * RDV_OBS_DIM);
  V* ws = reinterpret_cast<V*>(A.ws);

  Env e;
  if (active) load_env<ST>(ws, A.cs, i, e);
  uint64_t* slot = A.stats + (uint64_t)(wave_base / kWave) * kStatWords;
  const uint64_t slot_pre = rows > 0 ? stats_preload(slot, lane) : 0ull;
  float a[RDV_ACT_DIM];
  load_actions(A.actions, wave_base, lane, active, a);

  StepResult r;
  const RowSink my_row{wl + lane * RDV_OBS_DIM};
  const bool stepped = advance<ST, kDiag, false, kRaw>(A, P, i, active, e, a, r, my_row);
  const bool fin = stepped && r.done;
  stats_update(slot, slot_pre, lane, stepped, fin, r.reason, e.flags, e.k, e.ep_ret, e.sum_dv, e.sum_dw);
  store_step_outputs<true>(A, i, active, fin, r, e, my_row.row);
  bool did_reset = false;
  if (fin) {
    if (A.on_done == RDV_ON_DONE_RESET) {
      const double* row = nullptr;
      if (A.tape_depth > 0) row = A.tape + ((int64_t)(e.episode % (uint32_t)A.tape_depth) * n + i) * RDV_STATE_DIM;
      reset_env<ST>(P, e, A.seed, A.env_id_offset + (uint64_t)i, row);
      observation_to(P, e, my_row);
      did_reset = true;
    } else if (A.on_done == RDV_ON_DONE_HALT) {
      e.flags |= FLAG_HALTED;
    }
  }
  wave_lds_fence();
  if (A.stream_rows) store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);
  else store_obs_rows<false>(A.obs, wave_base, rows, lane, wl);
  if (stepped) store_env<ST>(ws, A.cs, i, e, did_reset);
}

// ---------------------------------------------------------------------------------------------------------------
// The cold kernels: one lane per env, 256-thread workgroups in env order, so blockIdx.x is the tile (rdv_cold.h has the bodies).
template <typename ST>
__global__ __launch_bounds__(kBlock) void reset_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, const StepArgs A,
                                                              const uint8_t* mask, float* obs, int fresh) {
  reset_lane<ST>(group_block(Pp, tile_group, blockIdx.x), A, mask, obs, fresh);
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void access_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, void* ws_, int64_t n,
                                                               int64_t cs, int what, const double* in, double* out, float* out_f32) {
  access_lane<ST>(group_block(Pp, tile_group, blockIdx.x), ws_, n, cs, what, in, out, out_f32);
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void eval_summary_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, const void* ws_,
                                                                     int64_t n, int64_t cs, const double* eval, double* partial) {
  eval_summary_lane<ST>(group_block(Pp, tile_group, blockIdx.x), ws_, n, cs, eval, partial);
}

// ---------------------------------------------------------------------------------------------------------------
#define RDV_LAUNCH_GR(GRID, ...) do { hipLaunchKernelGGL((__VA_ARGS__), GRID, dim3(kBlock), 0, s, A.ws, A.actions, T.params, A.n, A.stats, A.obs, A.reward, \
                                                         T.tile_group, A); return #__VA_ARGS__; } while (0)
const char* launch_step_groups(bool f32, bool all, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A) {
  if (f32) { if (all) RDV_LAUNCH_GR(grid, step_kernel_groups<float, true>); else RDV_LAUNCH_GR(grid, step_kernel_groups<float, false>); }
  else { if (all) RDV_LAUNCH_GR(grid, step_kernel_groups<double, true>); else RDV_LAUNCH_GR(grid, step_kernel_groups<double, false>); }
}
const char* launch_step_groups_lane(bool f32, bool diag, bool raw, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A) {
  if (f32) {
    if (raw) { if (diag) RDV_LAUNCH_GR(grid, step_kernel_groups_lane<float, true, true>); else RDV_LAUNCH_GR(grid, step_kernel_groups_lane<float, false, true>); }
    RDV_LAUNCH_GR(grid, step_kernel_groups_lane<float, true, false>);
  }
  if (raw) { if (diag) RDV_LAUNCH_GR(grid, step_kernel_groups_lane<double, true, true>); else RDV_LAUNCH_GR(grid, step_kernel_groups_lane<double, false, true>); }
  RDV_LAUNCH_GR(grid, step_kernel_groups_lane<double, true, false>);
}
#undef RDV_LAUNCH_GR
void launch_reset_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A, const uint8_t* mask, float* obs, int fresh) {
  if (f32) hipLaunchKernelGGL(reset_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, A, mask, obs, fresh);
  else hipLaunchKernelGGL(reset_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, A, mask, obs, fresh);
}
void launch_access_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, void* ws, int64_t n, int64_t cs, int what, const double* in, double* out,
                          float* out_f32) {
  if (f32) hipLaunchKernelGGL(access_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, what, in, out, out_f32);
  else hipLaunchKernelGGL(access_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, what, in, out, out_f32);
}
void launch_eval_summary_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const void* ws, int64_t n, int64_t cs, const double* eval, double* partial) {
  if (f32) hipLaunchKernelGGL(eval_summary_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, eval, partial);
  else hipLaunchKernelGGL(eval_summary_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, eval, partial);
}

}  // namespace rdv

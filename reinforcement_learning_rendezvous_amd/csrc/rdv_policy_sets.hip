// rdv_policy_sets.hip — the set forms of the eight actor / critic kernels (rdv_policy_sets.h): policy_set_act_kernel and
// policy_set_value_kernel for the shipped 17-64-64 tanh block, mlp_set_kernel<ACT, CRITIC> for the blocks of rdv_policy_mlp.h.  A
// translation unit of its own, as rdv_groups.hip and rdv_policy_mlp.hip are: the objects of rdv_hip.hip and rdv_policy_mlp.hip stay what
// they were.  The bodies are those of policy_act_kernel, policy_value_kernel and mlp_kernel with two differences: the parameter block a
// workgroup stages is its member's (one scalar load from the tile table, wave-uniform), and the critics address their rows as
// (row block blockIdx.y, tile blockIdx.x).  Every wave still reaches the one __syncthreads() before the nrows <= 0 exit.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy_mlp.h"
#include "rdv_policy_sets.h"

namespace rdv {

static_assert(kSetTile == kPolBlockEnvs, "a workgroup of the actor kernels owns one tile of the table");

// stage_obs_rows for a wave whose source address may be off the 16-byte grid (row block y of a critic over [k, n] rows with
// y * n % 4 != 0): a full wave then takes the element path, which stage_obs_rows itself only takes for a ragged wave.
__device__ __forceinline__ void stage_obs_rows_any(const float* __restrict__ obs, int64_t wave_base, int64_t nrows, float* rows, int lane) {
  const bool aligned = (reinterpret_cast<uintptr_t>(obs + wave_base * kPolIn) & 15u) == 0;   // wave-uniform
  if (aligned || nrows != kPolWaveEnvs) {
    stage_obs_rows(obs, wave_base, nrows, rows, lane);
  } else {
    const float* src = obs + wave_base * kPolIn;
    for (int j = 0; j < 9; ++j) {
      const int idx = j * 64 + lane;
      if (idx < kPolObsStage) rows[idx] = src[idx];
    }
  }
}

__global__ __launch_bounds__(kPolBlock) void policy_set_act_kernel(const float* __restrict__ W, const int32_t* __restrict__ tile_member,
                                                                   const float* __restrict__ obs, float* __restrict__ actions, int64_t n,
                                                                   int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset,
                                                                   float* __restrict__ raw_actions, float* __restrict__ log_prob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [parameters][8 x obs rows][8 x action rows]
  float* w = lds;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  float* rows = lds + kPolFloats + wv * kPolObsStage;
  float* arows = lds + kPolFloats + (kPolBlock / 64) * kPolObsStage + wv * kPolActStage;
  const int64_t wave_base = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_base) < kPolWaveEnvs ? (n - wave_base) : kPolWaveEnvs;   // <= 0 for trailing waves of the last workgroup
  const float* Wm = W + (size_t)tile_member[blockIdx.x] * kPolFloats;                       // this tile's member
  for (int q = threadIdx.x; q < kPolFloats / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(Wm + 4 * q);
  stage_obs_rows(obs, wave_base, nrows, rows, lane);
  __syncthreads();   // the parameters are in LDS (the only workgroup barrier; every wave reaches it)
  if (nrows <= 0) return;

  float a[4];
  if (wv < 4) __builtin_amdgcn_s_setprio(1);
  actor_means(w, rows, lane, a);
  if (wv < 4) __builtin_amdgcn_s_setprio(0);
  actor_outputs(w + kPolStd, lane, wave_base, nrows, deterministic, seed, counter, env_id_offset, a, arows, actions, raw_actions, log_prob);
}

// obs [gridDim.y, n, 17] -> values [gridDim.y, n]
__global__ __launch_bounds__(kPolBlock) void policy_set_value_kernel(const float* __restrict__ W, const int32_t* __restrict__ tile_member,
                                                                     const float* __restrict__ obs, float* __restrict__ values, int64_t n) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* w = lds;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  float* rows = lds + kPolFloats + wv * kPolObsStage;
  const int64_t wave_env = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_env) < kPolWaveEnvs ? (n - wave_env) : kPolWaveEnvs;
  const int64_t wave_base = (int64_t)blockIdx.y * n + wave_env;                            // flat row of the wave's first env
  const float* Wm = W + (size_t)tile_member[blockIdx.x] * kPolFloats;
  for (int q = threadIdx.x; q < kPolFloats / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(Wm + 4 * q);
  stage_obs_rows_any(obs, wave_base, nrows, rows, lane);
  __syncthreads();
  if (nrows <= 0) return;
  float v[4];
  actor_means(w, rows, lane, v);
  if (lane < nrows) values[wave_base + lane] = v[0];   // lanes 0..31: row 0 of the head tile of env l
}

// mlp_kernel for a set: `stride` = floats of one member's block (every member has the spec of the set, so the same size and H[3]); the
// layer table is read from the member's own block.  CRITIC: obs [gridDim.y, n, 17] -> out [gridDim.y, n]; the actor is launched with
// gridDim.y = 1.
template <int ACT, bool CRITIC>
__global__ __launch_bounds__(kPolBlock) __attribute__((amdgpu_waves_per_eu(4))) void mlp_set_kernel(const float* __restrict__ W, const int32_t* __restrict__ tile_member, int stride,
                                                        const float* __restrict__ obs, float* __restrict__ out,
                                                        int64_t n, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset,
                                                        float* __restrict__ raw_actions, float* __restrict__ log_prob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [parameters][8 x obs rows][8 x action rows]
  const float* Wm = W + (size_t)tile_member[blockIdx.x] * (size_t)stride;
  const int32_t* H = reinterpret_cast<const int32_t*>(Wm);
  const int total = H[3];
  float* w = lds;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  float* rows = lds + total + wv * kPolObsStage;
  float* arows = lds + total + (kPolBlock / 64) * kPolObsStage + wv * kPolActStage;
  const int64_t wave_env = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_env) < kPolWaveEnvs ? (n - wave_env) : kPolWaveEnvs;   // <= 0 for trailing waves of the last workgroup
  const int64_t wave_base = CRITIC ? (int64_t)blockIdx.y * n + wave_env : wave_env;
  for (int q = threadIdx.x; q < total / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(Wm + 4 * q);
  if (CRITIC) stage_obs_rows_any(obs, wave_base, nrows, rows, lane);
  else stage_obs_rows(obs, wave_base, nrows, rows, lane);
  __syncthreads();   // the parameters are in LDS (the only workgroup barrier; every wave reaches it)
  if (nrows <= 0) return;
  float a[4];
  mlp_means<ACT>(w, H, rows, lane, a);
  if (CRITIC) {
    if (lane < nrows) out[wave_base + lane] = a[0];   // lanes 0..31: row 0 of the head tile of env l
  } else {
    actor_outputs(w + kMlpStd, lane, wave_base, nrows, deterministic, seed, counter, env_id_offset, a, arows, out, raw_actions, log_prob);
  }
}

template <bool CRITIC>
static const void* mlp_set_kernel_of(int activation) {
  switch (activation) {
    case RDV_ACT_RELU: return reinterpret_cast<const void*>(mlp_set_kernel<RDV_ACT_RELU, CRITIC>);
    case RDV_ACT_SIGMOID: return reinterpret_cast<const void*>(mlp_set_kernel<RDV_ACT_SIGMOID, CRITIC>);
    default: return reinterpret_cast<const void*>(mlp_set_kernel<RDV_ACT_TANH, CRITIC>);
  }
}

hipError_t sets_raise_lds_limit(bool shipped_arch) {
  if (shipped_arch) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_set_act_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPolLdsBytes);
    if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_set_value_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPolLdsBytes);
    return err;
  }
  for (int act = 0; act < 3; ++act) {
    hipError_t err = hipFuncSetAttribute(mlp_set_kernel_of<false>(act), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpMaxLdsBytes);
    if (err == hipSuccess) err = hipFuncSetAttribute(mlp_set_kernel_of<true>(act), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpMaxLdsBytes);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

static inline unsigned set_tiles(int64_t rows) { return (unsigned)((rows + kSetTile - 1) / kSetTile); }

template <int ACT, bool CRITIC>
static void launch(const float* W, int block_floats, const int32_t* tile_member, const float* obs, float* out, int64_t rows, unsigned row_blocks,
                   int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  hipLaunchKernelGGL((mlp_set_kernel<ACT, CRITIC>), dim3(set_tiles(rows), row_blocks), dim3(kPolBlock), mlp_lds_bytes(block_floats), s, W, tile_member,
                     block_floats, obs, out, rows, deterministic, seed, counter, env_id_offset, raw_actions, log_prob);
}

void sets_launch_act(bool shipped_arch, int activation, const float* W, int block_floats, const int32_t* tile_member, const float* obs,
                     float* actions, int64_t rows, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset,
                     float* raw_actions, float* log_prob, hipStream_t s) {
  if (shipped_arch) {
    hipLaunchKernelGGL(policy_set_act_kernel, dim3(set_tiles(rows)), dim3(kPolBlock), kPolLdsBytes, s, W, tile_member, obs, actions, rows,
                       deterministic, seed, counter, env_id_offset, raw_actions, log_prob);
    return;
  }
  switch (activation) {
    case RDV_ACT_RELU: launch<RDV_ACT_RELU, false>(W, block_floats, tile_member, obs, actions, rows, 1, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
    case RDV_ACT_SIGMOID: launch<RDV_ACT_SIGMOID, false>(W, block_floats, tile_member, obs, actions, rows, 1, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
    default: launch<RDV_ACT_TANH, false>(W, block_floats, tile_member, obs, actions, rows, 1, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
  }
}

void sets_launch_value(bool shipped_arch, int activation, const float* W, int block_floats, const int32_t* tile_member, const float* obs,
                       float* values, int64_t rows, int64_t row_blocks, hipStream_t s) {
  for (int64_t y0 = 0; y0 < row_blocks; y0 += kSetMaxRowBlocks) {
    const unsigned ny = (unsigned)((row_blocks - y0) < kSetMaxRowBlocks ? (row_blocks - y0) : kSetMaxRowBlocks);
    const float* o = obs + y0 * rows * kPolIn;
    float* v = values + y0 * rows;
    if (shipped_arch) {
      hipLaunchKernelGGL(policy_set_value_kernel, dim3(set_tiles(rows), ny), dim3(kPolBlock), kPolLdsBytes, s, W, tile_member, o, v, rows);
      continue;
    }
    switch (activation) {
      case RDV_ACT_RELU: launch<RDV_ACT_RELU, true>(W, block_floats, tile_member, o, v, rows, ny, 1, 0, 0, 0, nullptr, nullptr, s); break;
      case RDV_ACT_SIGMOID: launch<RDV_ACT_SIGMOID, true>(W, block_floats, tile_member, o, v, rows, ny, 1, 0, 0, 0, nullptr, nullptr, s); break;
      default: launch<RDV_ACT_TANH, true>(W, block_floats, tile_member, o, v, rows, ny, 1, 0, 0, 0, nullptr, nullptr, s); break;
    }
  }
}

}  // namespace rdv

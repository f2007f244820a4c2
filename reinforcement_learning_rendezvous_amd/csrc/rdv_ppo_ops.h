// rdv_ppo_ops.h — the small device functions the PPO gradient kernels of rdv_ppo.hip and rdv_ppo_mlp.hip share: the deterministic wave
// reductions, the wave's power-of-two scale, and the LDS operand tiles of the weight-gradient contraction.
#pragma once

#include "rdv_policy.h"

namespace rdv {

__device__ __forceinline__ float wave_sum(float v) {   // the same tree every time: deterministic
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}
// The wave's power-of-two scale for a tensor whose largest |entry| in this lane is `m`: S with (wave max) * S in [2^13, 2^14), and 1 / S.
// fmaxf drops NaNs, so a NaN entry does not decide the scale (it stays a NaN through the split and the products); all zeros: S = 2^126.
__device__ __forceinline__ void wave_scale(float m, float& S, float& invS) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
  const int e = (int)((__float_as_uint(m) >> 23) & 0xffu);
  int se = 127 + 13 - (e - 127);
  se = se < 2 ? 2 : (se > 253 ? 253 : se);
  S = __uint_as_float((uint32_t)se << 23);
  invS = __uint_as_float((uint32_t)(254 - se) << 23);
}
__device__ __forceinline__ float tile_max(const float (&v)[16]) {
  float m = 0.0f;
#pragma unroll
  for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(v[e]));
  return m;
}
// A tile in accumulator order (lane = row r, register e = feature (e & 3) + 8 (e >> 2) + 4 h) -> the LDS operand tile [term][feature][row]
__device__ __forceinline__ void stage_tile(_Float16* tile, const float (&v)[16], int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int f = (e & 3) + 8 * (e >> 2) + 4 * h;
    const _Float16 hi = (_Float16)v[e];
    const _Float16 lo = (_Float16)(v[e] - (float)hi);
    tile[f * 32 + r] = hi;
    tile[32 * 32 + f * 32 + r] = lo;
  }
}
// the fragments of both k-steps (rows 16 s + 8 h + j) of a staged tile: lane (feature r, h) reads 16 bytes per term and k-step
__device__ __forceinline__ void load_frags(const _Float16* tile, int lane, f16x8 (&f)[2][2]) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int q = 0; q < 2; ++q) f[s][q] = *reinterpret_cast<const f16x8*>(tile + q * 32 * 32 + r * 32 + 16 * s + 8 * h);
}

}  // namespace rdv

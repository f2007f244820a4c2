// rdv_ppo_ops.h — everything the PPO gradient kernels of rdv_ppo.hip (the shipped architecture) and rdv_ppo_mlp.hip (every architecture)
// share, each piece defined once: the row arguments of a call, a wave's LDS share, the gather of a wave's rows, the loss terms of a
// lane's row (the clip, tie and NaN rules), the kept activation, the error fragments, the layer-0 input tile, the weight-gradient
// contraction through the LDS operand tiles with its sum in wave order, the workgroup's scalar sums, the double-precision tail of the
// last kernel, the index arithmetic of the transposed fragments, and the wave reductions, wave scale and tile staging under them.  The
// order of the floating-point operations, the barriers and the summation orders here fix the output bits (tests/test_gpu_ppo_digests.py).
#pragma once

#include "rdv_policy_mlp.h"

namespace rdv {

// ---- the rows of one call, as every net kernel takes them (embedded in its argument struct)
struct PpoRowArgs {
  const float *obs, *actions, *old_log_prob, *advantages, *returns;
  const int64_t* indices;                    // nullable
  int64_t n;
  float clip_lo, clip_hi, clip_range, vf2;   // (float)(1 - eps), (float)(1 + eps), (float)eps; vf2 = 2 vf_coef
};
template <class Launch>   // PpoLaunch, PpoMlpLaunch: the same field names
inline PpoRowArgs ppo_row_args(const Launch& a) {
  return {a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, a.indices, a.n, a.k.clip_lo, a.k.clip_hi, a.k.clip_range, 2.0f * a.k.vf_coef};
}

// ---- LDS.  An operand tile is [term hi, lo][feature 32][row 32] fp16 = 4 KiB = 1,024 floats; tiles 0, 1 of a wave hold the B operand
// (the layer's input, up to 64 features), tile 2 the A operand (32 features of delta_l) and then, as [32][32] fp32, the wave's product of
// that tile.  A wave's share of the workgroup's LDS: its observation rows [32][17], its three tiles, its 4 scalar sums = 14,480 B.
constexpr int kPpoTile = 1024, kPpoWaveTiles = 3 * kPpoTile;
constexpr int kPpoWaveFloats = kPolObsStage + kPpoWaveTiles + 4;

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

// ---- the transposed fragments.  Backward fragment k-step ks, lane (r, h), element j of input tile mt holds W[o][i], o = perm(ks, h, j)
// of rdv_policy.h, i = 32 mt + r; the forward block keeps it in tile row o >> 5, k-step ks_i, lane (o & 31, h_i), element j_i: perm's inverse.
struct PpoTransposeIndex { int o, i, ks_i, h_i, j_i; };
__device__ __forceinline__ PpoTransposeIndex ppo_transpose_index(int ks, int h, int j, int mt, int r) {
  const int o = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3), i = 32 * mt + r;
  return {o, i, (i >> 5) * 2 + ((i >> 4) & 1), (i >> 2) & 1, ((i >> 3) & 1) * 4 + (i & 3)};
}

// ---- the wave's observation rows -> its LDS rows, contiguous (stage_obs_rows) or through `indices` (missing rows = 0: finite
// activations, and their errors are zero).  valid: this lane's row exists; returns its row of the call's columns.  The caller's barrier follows.
__device__ __forceinline__ int64_t ppo_gather_rows(const PpoRowArgs& A, int64_t wave_base, int nrows, float* rows, int lane, bool& valid) {
  if (!A.indices && nrows > 0) {
    stage_obs_rows(A.obs, wave_base, nrows, rows, lane);
  } else {
    for (int j = 0; j < 9; ++j) {
      const int idx = j * 64 + lane;
      if (idx < kPolObsStage) {
        const int row = idx / kPolIn, col = idx - row * kPolIn;
        rows[idx] = row < nrows ? A.obs[A.indices[wave_base + row] * kPolIn + col] : 0.0f;
      }
    }
  }
  const int r = lane & 31;
  valid = r < nrows;
  return valid ? (A.indices ? A.indices[wave_base + r] : wave_base + r) : 0;
}

// ---- the loss terms of this lane's row (sample `row` of the minibatch, row `src` of the columns) from the head's outputs `mean`: the
// head's error (times n) in d3, the d log_std terms in ex (actor), the wave's four scalar sums -> red4 (policy, kl, clipped count |
// value), log_prob (actor) or the value (critic) -> out[row] (out nullable).  sd, lsd: exp(log_std) and log_std in LDS.
template <bool ACTOR>
__device__ __forceinline__ void ppo_loss_terms(const PpoRowArgs& A, const float* sd, const float* lsd, const float (&mean)[4], bool valid, int64_t src,
                                               float* out, int64_t row, int lane, float* red4, float (&d3)[4], float (&ex)[4]) {
  const int h = lane >> 5;
  float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 4; ++c) { d3[c] = 0.0f; ex[c] = 0.0f; }
  if constexpr (ACTOR) {
    float dm[4], dl[4], lp = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool comp = valid && (h == 0 || c < 2);                     // the upper half holds components 4, 5 only
      const float act = comp ? A.actions[src * kPolOut + 4 * h + c] : mean[c];
      const float sdv = comp ? sd[4 * h + c] : 1.0f, ls = comp ? lsd[4 * h + c] : 0.0f;
      const float var = sdv * sdv, d = act - mean[c], t = d * d / (2.0f * var);
      lp += comp ? (-t - ls) : 0.0f;
      dm[c] = comp ? d / var : 0.0f;                                   // d log_prob / d mean_c
      dl[c] = comp ? 2.0f * t - 1.0f : 0.0f;                           // d log_prob / d log_std_c
    }
    lp = (lp + __shfl_xor(lp, 32)) - 5.5136312f;                        // - 6/2 log(2 pi)
    float g = 0.0f;
    if (valid) {
      const float old = A.old_log_prob[src], adv = A.advantages[src];
      const float diff = lp - old, ratio = expf(diff);
      const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, A.clip_lo), A.clip_hi);
      // PyTorch's backward of min(s1, s2) and clamp (the rule of include/rdv.h): a tie halves the gradient between the two, clamp passes it
      // inside the inclusive limits; comparisons with a NaN are false, so a NaN row keeps its gradient path and poisons the sums
      const float g1 = s1 == s2 ? 0.5f : (s1 > s2 ? 0.0f : 1.0f), g2 = s1 == s2 ? 0.5f : (s2 > s1 ? 0.0f : 1.0f);
      const float gc = (ratio >= A.clip_lo && ratio <= A.clip_hi) ? 1.0f : 0.0f;
      g = -(adv * (g1 + g2 * gc)) * ratio;                              // d (n policy_loss) / d log_prob
      if (h == 0) {
        sums[0] = -((s1 < s2 || s1 != s1) ? s1 : s2);
        sums[1] = (ratio - 1.0f) - diff;
        sums[2] = fabsf(ratio - 1.0f) > A.clip_range ? 1.0f : 0.0f;
        if (out) out[row] = lp;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { d3[c] = g * dm[c]; ex[c] = g * dl[c]; }
  } else {
    if (valid && h == 0) {
      const float diff = mean[0] - A.returns[src];
      d3[0] = A.vf2 * diff;
      sums[3] = diff * diff;
      if (out) out[row] = mean[0];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sums[k] = (ACTOR ? k < 3 : k == 3) ? wave_sum(sums[k]) : 0.0f;   // (the other net's sums are zeros: no shuffles for them)
  if (lane == 0) { red4[0] = sums[0]; red4[1] = sums[1]; red4[2] = sums[2]; red4[3] = sums[3]; }
}
// the workgroup's scalar sums (red[] behind a barrier), its nw waves in order -> dst[0..2] (actor) or dst[3] (critic)
template <bool ACTOR>
__device__ __forceinline__ void ppo_store_scalar_sums(const float* red, int nw, float* dst) {
  if (threadIdx.x < 4 && (ACTOR ? threadIdx.x < 3 : threadIdx.x == 3)) {
    float sum = 0.0f;
    for (int k = 0; k < nw; ++k) sum += red[k * 4 + threadIdx.x];
    dst[threadIdx.x] = sum;
  }
}

// ---- mlp_activate of rdv_policy_mlp.h (tanh: `activate` of rdv_policy.h), the same operations in the same order, that also keeps the activations (times 2^10)
template <int ACT>
__device__ __forceinline__ void ppo_activate_keep(const f32x16& d, float k, f16x8 (&lo_step)[2], f16x8 (&hi_step)[2], float (&hs)[16]) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; j += 2) mlp_act2<ACT>(d[j], d[j + 1], k, x[j], x[j + 1]);
  split2(x, lo_step);
#pragma unroll
  for (int j = 0; j < 8; ++j) hs[j] = x[j];
#pragma unroll
  for (int j = 0; j < 8; j += 2) mlp_act2<ACT>(d[8 + j], d[9 + j], k, x[j], x[j + 1]);
  split2(x, hi_step);
#pragma unroll
  for (int j = 0; j < 8; ++j) hs[8 + j] = x[j];
}
// registers 8 s .. 8 s + 7 of an error tile (accumulator order, already scaled) as the B fragments of k-step s of the next backward layer
__device__ __forceinline__ void error_frags(const float (&v)[16], int s, f16x8 (&step)[2]) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = v[8 * s + j];
  split2(x, step);
}
// layer 0's B operand in accumulator order: the wave's staged observation rows as the forward pass reads them (times 2^10, clamped to
// +-63, a NaN kept).  The caller stages it (stage_tile -> its tile 0): with stage_tile inside this function the compiler added ~11
// address instructions per call and the 4 x 64 net measured 2 us per call slower (profiles/ppo_shared_isa_diff.md).
__device__ __forceinline__ void ppo_input_tile(const float* rows, int lane, float (&xin)[16]) {
  constexpr float xs = (float)(1 << kPolXShift), xmax = 63.0f * xs;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int f = (e & 3) + 8 * (e >> 2) + 4 * h;
    const float v = f < kPolIn ? rows[r * kPolIn + f] : 0.0f;
    const float cl = __builtin_amdgcn_fmed3f(v * xs, -xmax, xmax);
    xin[e] = v != v ? v : cl;
  }
}

// ---- dW = delta . B^T for one layer: MT row tiles of delta (accumulator order, scaled by the wave's S), NT staged B tiles (this wave's
// tiles 0 .. NT-1, features times 2^10) and one more column tile of ones (times 2^10), whose column 0 holds the row sums (bias gradients).
// Per (mt, nt): the wave's product, unscaled, -> its tile 2 as [32][32] fp32; barrier; the workgroup's waves' tiles added in wave order,
// element (row 32 mt + m, column 32 nt + c) handed to store(row, col, sum) (the ones tile: store(row, -1 - c, sum)); barrier.
// Every wave of the workgroup takes part.  NW: the workgroup's waves, or 0 for the run-time count `nw`.
template <int MT, int NT, int NW, int D, class Store>
__device__ __forceinline__ void weight_grads(const float (&delta)[D][16], float* wave_tiles, const float* tiles0, int nw, float unscale, int lane, Store store) {
  if (NW) nw = NW;
  _Float16* tb = reinterpret_cast<_Float16*>(wave_tiles);
  float* prod = wave_tiles + 2 * kPpoTile;
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    stage_tile(tb + 2 * (2 * kPpoTile), delta[mt], lane);
    wave_fence();
    f16x8 a[2][2];
    load_frags(tb + 2 * (2 * kPpoTile), lane, a);
#pragma unroll
    for (int nt = 0; nt <= NT; ++nt) {
      f16x8 b[2][2];
      if (nt < NT) {
        load_frags(tb + nt * (2 * kPpoTile), lane, b);
      } else {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) { b[s][0][j] = (_Float16)(float)(1 << kPolXShift); b[s][1][j] = (_Float16)0.0f; }
      }
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
      acc = mfma3(a[0], b[0], acc);
      acc = mfma3(a[1], b[1], acc);
      wave_fence();
#pragma unroll
      for (int e = 0; e < 16; ++e) prod[((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + c] = acc[e] * unscale;
      __syncthreads();
      for (int el = (int)threadIdx.x, k = 0; NW ? k * NW * 64 < kPpoTile : el < kPpoTile; el += nw * 64, ++k) {   // NW: a compile-time trip count, unrolled
        float sum = 0.0f;
        for (int wv = 0; wv < nw; ++wv) sum += tiles0[wv * kPpoWaveTiles + 2 * kPpoTile + el];
        store(32 * mt + (el >> 5), nt < NT ? 32 * nt + (el & 31) : -1 - (el & 31), sum);
      }
      __syncthreads();
    }
  }
}

// ---- the tail of the last kernel, one thread: from the four scalar sums (in double, workgroups in index order) the eight output scalars
__device__ __forceinline__ void ppo_finish_scalars(const double (&s)[4], int64_t n, const float* log_std, float ent_coef, float vf_coef, float* scalars) {
  const double dn = (double)n, policy = s[0] / dn, value = s[3] / dn;
  double entropy = 0.0;
  for (int c = 0; c < kPolOut; ++c) entropy += 0.5 + 0.5 * 1.8378770664093453 + (double)log_std[c];
  const double entropy_loss = -entropy;
  scalars[0] = (float)(policy + (double)ent_coef * entropy_loss + (double)vf_coef * value);
  scalars[1] = (float)policy; scalars[2] = (float)value; scalars[3] = (float)entropy_loss;
  scalars[4] = (float)(s[1] / dn); scalars[5] = (float)(s[2] / dn); scalars[6] = 0.0f; scalars[7] = 0.0f;
}

}  // namespace rdv

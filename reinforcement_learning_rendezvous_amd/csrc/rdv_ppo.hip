// rdv_ppo.hip — the kernels of rdv_ppo.h and their launch, in a translation unit of its own (the objects of the other units do not change
// when it does).  The exported rdv_ppo_* entry points are in rdv_policy_host.hip, with the other policy entry points.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_ppo.h"
#include "rdv_ppo_ops.h"

#include <type_traits>

namespace rdv {

// LDS of ppo_net_kernel (floats): parameters | per wave: observation rows [32][17] | per wave: three operand tiles | per wave: 4 scalar sums.
// An operand tile is [term hi, lo][feature 32][row 32] fp16 = 4 KiB = 1,024 floats; tiles 0, 1 of a wave hold the B operand (h_{l-1}, 64
// features), tile 2 the A operand (32 features of delta_l) and then, as [32][32] fp32, the wave's product of that tile.
constexpr int kPpoTile = 1024, kPpoWaveTiles = 3 * kPpoTile, kPpoWaves = kPolBlock / 64;
constexpr int kPpoLdsObs = kPolFloats, kPpoLdsTiles = kPpoLdsObs + kPpoWaves * kPolObsStage, kPpoLdsRed = kPpoLdsTiles + kPpoWaves * kPpoWaveTiles;
constexpr int kPpoLdsBytes = (kPpoLdsRed + kPpoWaves * 4) * 4;   // 149,328 B: one workgroup per CU
static_assert(kPpoLdsBytes <= 160 * 1024, "the workgroup's LDS");
static_assert(kPpoBlockRows == kPolBlockEnvs, "a workgroup owns 256 rows");

// ---- 1. the transposed fragments.  Backward fragment b of a net, lane (r, h), element j (k order of an accumulator tile used as B
// operand: perm(ks, h, j) of rdv_policy.h):
//   W3^T, b = q*2 + mt            : W3_q[perm(0, h, j)][32 mt + r]          (rows >= out_dim of the forward head tile are zero)
//   W2^T, b = 4 + (q*2 + mt)*4 + ks: W2_q[perm(ks, h, j)][32 mt + r]
// read from where the forward block keeps W_q[o][i]: fragment base + (q*MT + (o >> 5))*4 + ks(i), lane (o & 31, h(i)), element j(i), the
// inverse of perm.
__device__ __forceinline__ void ppo_transpose_body(const uint16_t* __restrict__ src, float* __restrict__ dstf) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b == kPpoBwdFrags) { if (t < 64) dstf[kPpoBwdZero + t] = 0.0f; return; }
  const int lane = t >> 3, j = t & 7, r = lane & 31, h = lane >> 5;
  const bool head = b < kPpoBwdW2;
  const int bb = head ? b : b - kPpoBwdW2;
  const int q = head ? bb >> 1 : bb >> 3, mt = head ? bb & 1 : (bb >> 2) & 1, ks = head ? 0 : bb & 3;
  const int o = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3), i = 32 * mt + r;
  const int ks_i = (i >> 5) * 2 + ((i >> 4) & 1), h_i = (i >> 2) & 1, j_i = ((i >> 3) & 1) * 4 + (i & 3);
  const int frag = head ? kPolW3Frag + q * 4 + ks_i : kPolW2Frag + (q * 2 + (o >> 5)) * 4 + ks_i;
  reinterpret_cast<uint16_t*>(dstf)[(b * 64 + lane) * 8 + j] = src[(frag * 64 + (o & 31) + 32 * h_i) * 8 + j_i];
}
__global__ __launch_bounds__(512) void ppo_transpose_kernel(const float* __restrict__ actor_block, const float* __restrict__ critic_block,
                                                            float* __restrict__ workspace) {
  ppo_transpose_body(reinterpret_cast<const uint16_t*>(blockIdx.y == 0 ? actor_block : critic_block), workspace + (size_t)blockIdx.y * kPpoBwdFloats);
}
// the set form: member blockIdx.z of the sets' allocations -> the head of its piece of the workspace; a member without samples is skipped
__global__ __launch_bounds__(512) void ppo_set_transpose_kernel(const float* __restrict__ actor_set, const float* __restrict__ critic_set,
                                                                float* __restrict__ workspace, const PpoSetTable T) {
  const int g = blockIdx.z;
  if (T.count[g] == 0) return;
  const float* block = (blockIdx.y == 0 ? actor_set : critic_set) + (size_t)g * kPolFloats;
  ppo_transpose_body(reinterpret_cast<const uint16_t*>(block), workspace + T.ws[g] + (size_t)blockIdx.y * kPpoBwdFloats);
}

// ---- 2, 3. one net's loss terms and gradients
struct PpoNetArgs {
  const float *block, *bwd;      // forward parameter block, backward block (workspace)
  const float *obs, *actions, *old_log_prob, *advantages, *returns;
  const int64_t* indices;
  int64_t n;
  float clip_lo, clip_hi, clip_range, vf2;   // vf2 = 2 vf_coef
  float* parts;                  // [workgroups][kPpoPartFloats]
  float* out;                    // nullable [n]: log_prob (actor) or values (critic)
};

// tanh of a (scaled) accumulator tile as `activate` of rdv_policy.h takes it — the same operations in the same order — that also keeps the
// activations (times 2^10) for the backward pass
__device__ __forceinline__ void activate_keep(const f32x16& d, float kexp, f16x8 (&lo_step)[2], f16x8 (&hi_step)[2], float (&hs)[16]) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; j += 2) tanh2_f32(d[j], d[j + 1], kexp, x[j], x[j + 1]);
  split2(x, lo_step);
#pragma unroll
  for (int j = 0; j < 8; ++j) hs[j] = x[j];
#pragma unroll
  for (int j = 0; j < 8; j += 2) tanh2_f32(d[8 + j], d[9 + j], kexp, x[j], x[j + 1]);
  split2(x, hi_step);
#pragma unroll
  for (int j = 0; j < 8; ++j) hs[8 + j] = x[j];
}

// actor_means of rdv_policy.h with the hidden activations kept: hs1, hs2 [row tile][accumulator register], times 2^10
__device__ __forceinline__ void ppo_forward(const float* w, const float* rows, int lane, float (&hs1)[2][16], float (&hs2)[2][16], float (&mean)[4]) {
  f16x8 x0[2][2];
  actor_inputs(rows, lane, x0);
  constexpr float two_log2e = 2.8853900817779268f;
  f32x16 d1[2];
  layer<2, 2>(w, kPolW1Frag, w + kPolB1, x0, lane, d1);
  f16x8 x1[4][2];
  const float k1 = two_log2e * w[kPolScale + 0];
  activate_keep(d1[0], k1, x1[0], x1[1], hs1[0]);
  activate_keep(d1[1], k1, x1[2], x1[3], hs1[1]);
  f32x16 d2[2];
  layer<2, 4>(w, kPolW2Frag, w + kPolB2, x1, lane, d2);
  f16x8 x2[4][2];
  const float k2 = two_log2e * w[kPolScale + 1];
  activate_keep(d2[0], k2, x2[0], x2[1], hs2[0]);
  activate_keep(d2[1], k2, x2[2], x2[3], hs2[1]);
  f32x16 d3[1];
  layer<1, 4>(w, kPolW3Frag, w + kPolB3, x2, lane, d3);
  const float s3 = w[kPolScale + 2];
  mean[0] = d3[0][0] * s3; mean[1] = d3[0][1] * s3; mean[2] = d3[0][2] * s3; mean[3] = d3[0][3] * s3;
}

// an error tile (accumulator order, already scaled) as the B fragments of the next backward layer's k-steps 2 t, 2 t + 1
__device__ __forceinline__ void error_frags(const float (&v)[16], f16x8 (&lo_step)[2], f16x8 (&hi_step)[2]) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = v[j];
  split2(x, lo_step);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = v[8 + j];
  split2(x, hi_step);
}
// delta = pre o (1 - h^2) * unscale for one tile (hs = h * 2^10)
__device__ __forceinline__ void error_tile(const f32x16& pre, const float (&hs)[16], float unscale, float (&delta)[16]) {
  constexpr float inv = 1.0f / (float)(1 << kPolXShift);
#pragma unroll
  for (int e = 0; e < 16; ++e) { const float hv = hs[e] * inv; delta[e] = pre[e] * (1.0f - hv * hv) * unscale; }
}

// dW = delta . B^T for one layer: MT row tiles of delta (accumulator order, scaled by the wave's S), NT staged B tiles (this wave's tiles 0
// .. NT-1, features times 2^10) and one more column tile of ones (times 2^10), whose column 0 holds the row sums (bias gradients).
// Per (mt, nt): the wave's product, unscaled, -> its tile 2 as [32][32] fp32; barrier; the eight waves' tiles added in wave order, element
// (m, c) handed to store(mt, nt, m, c, sum) (nt == NT: the ones tile); barrier.  Every wave of the workgroup takes part.
template <int MT, int NT, class Store>
__device__ __forceinline__ void weight_grads(const float (&delta)[MT][16], float* wave_tiles, const float* tiles0, float unscale, int lane, Store store) {
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
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int el = (int)threadIdx.x + k * kPolBlock;
        float sum = 0.0f;
#pragma unroll
        for (int wv = 0; wv < kPpoWaves; ++wv) sum += tiles0[wv * kPpoWaveTiles + 2 * kPpoTile + el];
        store(mt, nt, el >> 5, el & 31, sum);
      }
      __syncthreads();
    }
  }
}

// The set form's arguments: `net` holds the set-wide pointers (block: the set's allocation; parts: the workspace; indices and out: all
// members'; bwd and n unused); ppo_member_args derives member blockIdx.y's own.  `idle`: workgroup x has no rows of that member (it has
// fewer workgroups than the widest member, or no samples) — a workgroup-uniform test, taken before the first barrier.
struct PpoSetNetArgs {
  PpoNetArgs net;
  PpoSetTable table;
};
template <bool ACTOR, bool SET>
__device__ __forceinline__ PpoNetArgs ppo_member_args(const std::conditional_t<SET, PpoSetNetArgs, PpoNetArgs>& S, bool& idle) {
  if constexpr (SET) {
    const int g = blockIdx.y;
    const int64_t n = S.table.count[g];
    idle = (int64_t)blockIdx.x * kPpoBlockRows >= n;
    const int64_t off = S.table.off[g];
    float* ws = S.net.parts + S.table.ws[g];
    PpoNetArgs M = S.net;
    M.block = S.net.block + (size_t)g * kPolFloats;
    M.bwd = ws + (ACTOR ? 0 : kPpoBwdFloats);
    M.indices = S.net.indices + off;
    M.n = n;
    M.parts = ws + 2 * kPpoBwdFloats;
    M.out = S.net.out ? S.net.out + off : nullptr;
    return M;
  } else {
    idle = false;
    return S;
  }
}
// SET = false: the kernel of rdv_ppo_loss_grad, the instruction stream it had before there was a set form (profiles/ppo_set_isa_diff.md).
// SET = true: workgroup (x, y) is workgroup x of member y's stand-alone launch: the same body on the member's arguments.
template <bool ACTOR, bool SET>
__global__ __launch_bounds__(kPolBlock) void ppo_net_kernel(const std::conditional_t<SET, PpoSetNetArgs, PpoNetArgs> S) {
  bool idle;
  const PpoNetArgs A = ppo_member_args<ACTOR, SET>(S, idle);
  if (SET && idle) return;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int OUT = ACTOR ? kPolOut : 1;
  float* w = lds;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  float* rows = lds + kPpoLdsObs + wv * kPolObsStage;
  float* tiles0 = lds + kPpoLdsTiles;
  float* wave_tiles = tiles0 + wv * kPpoWaveTiles;
  float* red = lds + kPpoLdsRed;
  const int64_t wave_base = ((int64_t)blockIdx.x * kPpoWaves + wv) * kPolWaveEnvs;
  const int64_t left = A.n - wave_base;
  const int nrows = left < 0 ? 0 : (left < kPolWaveEnvs ? (int)left : kPolWaveEnvs);   // trailing waves: 0 rows, and they stay (barriers below)

  for (int q = threadIdx.x; q < kPolFloats / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(A.block + 4 * q);

  // ---- the wave's observation rows (missing rows = 0: finite activations, and their errors are zero)
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
  const bool valid = r < nrows;
  const int64_t src = valid ? (A.indices ? A.indices[wave_base + r] : wave_base + r) : 0;
  __syncthreads();

  float hs1[2][16], hs2[2][16], mean[4];
  ppo_forward(w, rows, lane, hs1, hs2, mean);

  // ---- the loss terms of this lane's row: the head's error (times n) in d3, the d log_std terms in ex (actor), the scalar sums
  float d3[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ex[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (ACTOR) {
    const float* sd = w + kPolStd;
    float dm[4], dl[4], lp = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool comp = valid && (h == 0 || c < 2);                     // the upper half holds components 4, 5 only
      const float act = comp ? A.actions[src * kPolOut + 4 * h + c] : mean[c];
      const float sdv = comp ? sd[4 * h + c] : 1.0f, ls = comp ? sd[kPolLogStd - kPolStd + 4 * h + c] : 0.0f;
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
        if (A.out) A.out[wave_base + r] = lp;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { d3[c] = g * dm[c]; ex[c] = g * dl[c]; }
  } else {
    if (valid && h == 0) {
      const float diff = mean[0] - A.returns[src];
      d3[0] = A.vf2 * diff;
      sums[3] = diff * diff;
      if (A.out) A.out[wave_base + r] = mean[0];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sums[k] = wave_sum(sums[k]);
  if (lane == 0) { red[wv * 4 + 0] = sums[0]; red[wv * 4 + 1] = sums[1]; red[wv * 4 + 2] = sums[2]; red[wv * 4 + 3] = sums[3]; }

  const float* bwd = A.bwd;
  float* part = A.parts + (size_t)blockIdx.x * kPpoPartFloats + (ACTOR ? 0 : kPpoPartCritic);
  constexpr float xs = (float)(1 << kPolXShift), inv_xs = 1.0f / xs;

  // ---- head: scale, delta_2 = (W3^T delta_3) o (1 - h2^2), then dW3 / db3 / d log_std
  float S3, invS3;
  {
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) m = fmaxf(m, fmaxf(fabsf(d3[c]), fabsf(ex[c])));
    wave_scale(m, S3, invS3);
  }
  float head[1][16];
#pragma unroll
  for (int e = 0; e < 16; ++e) head[0][e] = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) { head[0][c] = d3[c] * S3; head[0][4 + c] = ex[c] * S3; }   // features 4 h + c, and 8 + 4 h + c
  float delta2[2][16];
  {
    float x[8] = {head[0][0], head[0][1], head[0][2], head[0][3], 0.0f, 0.0f, 0.0f, 0.0f};   // the d log_std terms stay out of the product
    f16x8 b3[1][2];
    split2(x, b3[0]);
    f32x16 pre[2];
    layer<2, 1>(bwd, kPpoBwdW3, bwd + kPpoBwdZero, b3, lane, pre);
    const float un = w[kPolScale + 2] * xs * invS3;                    // 2^-s3 / S3
    error_tile(pre[0], hs2[0], un, delta2[0]);
    error_tile(pre[1], hs2[1], un, delta2[1]);
  }
  {
    _Float16* tb = reinterpret_cast<_Float16*>(wave_tiles);
    stage_tile(tb, hs2[0], lane);
    stage_tile(tb + 2 * kPpoTile, hs2[1], lane);
    weight_grads<1, 2>(head, wave_tiles, tiles0, invS3 * inv_xs, lane, [&](int, int nt, int m, int c, float v) {
      if (nt < 2) { if (m < OUT) part[kPpoW3 + m * kPolHid + 32 * nt + c] = v; }
      else if (c == 0) {
        if (m < OUT) part[kPpoW3 + OUT * kPolHid + m] = v;
        if (ACTOR && m >= 8 && m < 8 + kPolOut) part[kPpoW3 + OUT * kPolHid + OUT + (m - 8)] = v;
      }
    });
  }
  // the workgroup's scalar sums (red[] is behind a barrier by now), waves in order
  if (threadIdx.x < 4 && (ACTOR ? threadIdx.x < 3 : threadIdx.x == 3)) {
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kPpoWaves; ++k) sum += red[k * 4 + threadIdx.x];
    A.parts[(size_t)blockIdx.x * kPpoPartFloats + kPpoPartScalars + threadIdx.x] = sum;
  }

  // ---- layer 2: delta_1 = (W2^T delta_2) o (1 - h1^2), dW2 / db2
  float S2, invS2;
  wave_scale(fmaxf(tile_max(delta2[0]), tile_max(delta2[1])), S2, invS2);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) delta2[mt][e] *= S2;
  float delta1[2][16];
  {
    f16x8 b2[4][2];
    error_frags(delta2[0], b2[0], b2[1]);
    error_frags(delta2[1], b2[2], b2[3]);
    f32x16 pre[2];
    layer<2, 4>(bwd, kPpoBwdW2, bwd + kPpoBwdZero, b2, lane, pre);
    const float un = w[kPolScale + 1] * xs * invS2;
    error_tile(pre[0], hs1[0], un, delta1[0]);
    error_tile(pre[1], hs1[1], un, delta1[1]);
  }
  {
    _Float16* tb = reinterpret_cast<_Float16*>(wave_tiles);
    stage_tile(tb, hs1[0], lane);
    stage_tile(tb + 2 * kPpoTile, hs1[1], lane);
    weight_grads<2, 2>(delta2, wave_tiles, tiles0, invS2 * inv_xs, lane, [&](int mt, int nt, int m, int c, float v) {
      if (nt < 2) part[kPpoW2 + (32 * mt + m) * kPolHid + 32 * nt + c] = v;
      else if (c == 0) part[kPpoB2 + 32 * mt + m] = v;
    });
  }

  // ---- layer 1: dW1 = delta_1 . x^T with the staged observation rows as the forward pass reads them (times 2^10, clamped to +-63), db1
  float S1, invS1;
  wave_scale(fmaxf(tile_max(delta1[0]), tile_max(delta1[1])), S1, invS1);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) delta1[mt][e] *= S1;
  {
    constexpr float xmax = 63.0f * xs;
    float xin[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int f = (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = f < kPolIn ? rows[r * kPolIn + f] : 0.0f;
      const float cl = __builtin_amdgcn_fmed3f(v * xs, -xmax, xmax);
      xin[e] = v != v ? v : cl;
    }
    stage_tile(reinterpret_cast<_Float16*>(wave_tiles), xin, lane);
    weight_grads<2, 1>(delta1, wave_tiles, tiles0, invS1 * inv_xs, lane, [&](int mt, int nt, int m, int c, float v) {
      if (nt < 1) { if (c < kPolIn) part[kPpoW1 + (32 * mt + m) * kPolIn + c] = v; }
      else if (c == 0) part[kPpoB1 + 32 * mt + m] = v;
    });
  }
}

// ---- 4. the workgroups' rows added in index order -> the gradients (divided by n; - ent_coef on d log_std) and the scalars
__device__ __forceinline__ void ppo_finish_body(const float* __restrict__ parts, int64_t workgroups, int64_t n, const float* __restrict__ actor_block,
                                                float ent_coef, float vf_coef, float* __restrict__ actor_grad, float* __restrict__ critic_grad,
                                                float* __restrict__ scalars) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float fn = (float)n;
  if (i < kPpoActorGrad + kPpoCriticGrad) {
    float sum = 0.0f;
    for (int64_t g = 0; g < workgroups; ++g) sum += parts[g * kPpoPartFloats + i];
    float v = sum / fn;
    if (i < kPpoActorGrad) {
      if (i >= kPpoActorGrad - kPolOut) v -= ent_coef;
      actor_grad[i] = v;
    } else {
      critic_grad[i - kPpoActorGrad] = v;
    }
  } else if (i == kPpoActorGrad + kPpoCriticGrad) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t g = 0; g < workgroups; ++g)
      for (int k = 0; k < 4; ++k) s[k] += (double)parts[g * kPpoPartFloats + kPpoPartScalars + k];
    const double dn = (double)n, policy = s[0] / dn, value = s[3] / dn;
    double entropy = 0.0;
    for (int c = 0; c < kPolOut; ++c) entropy += 0.5 + 0.5 * 1.8378770664093453 + (double)actor_block[kPolLogStd + c];
    const double entropy_loss = -entropy;
    scalars[0] = (float)(policy + (double)ent_coef * entropy_loss + (double)vf_coef * value);
    scalars[1] = (float)policy; scalars[2] = (float)value; scalars[3] = (float)entropy_loss;
    scalars[4] = (float)(s[1] / dn); scalars[5] = (float)(s[2] / dn); scalars[6] = 0.0f; scalars[7] = 0.0f;
  }
}
__global__ __launch_bounds__(256) void ppo_finish_kernel(const float* __restrict__ parts, int64_t workgroups, int64_t n, const float* __restrict__ actor_block,
                                                          float ent_coef, float vf_coef, float* __restrict__ actor_grad, float* __restrict__ critic_grad,
                                                          float* __restrict__ scalars) {
  ppo_finish_body(parts, workgroups, n, actor_block, ent_coef, vf_coef, actor_grad, critic_grad, scalars);
}
// the set form: member blockIdx.y's rows of the workspace -> row blockIdx.y of the outputs; nothing of a member without samples is written
__global__ __launch_bounds__(256) void ppo_set_finish_kernel(const float* __restrict__ workspace, const float* __restrict__ actor_set, float ent_coef,
                                                              float vf_coef, float* __restrict__ actor_grad, float* __restrict__ critic_grad,
                                                              float* __restrict__ scalars, const PpoSetTable T) {
  const int g = blockIdx.y;
  const int64_t n = T.count[g];
  if (n == 0) return;
  ppo_finish_body(workspace + T.ws[g] + 2 * kPpoBwdFloats, (n + kPpoBlockRows - 1) / kPpoBlockRows, n, actor_set + (size_t)g * kPolFloats, ent_coef, vf_coef,
                  actor_grad + (size_t)g * kPpoActorGrad, critic_grad + (size_t)g * kPpoCriticGrad, scalars + (size_t)g * kPpoScalars);
}

hipError_t ppo_raise_lds_limit() {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_net_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kPpoLdsBytes);
  if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_net_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kPpoLdsBytes);
  if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_net_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kPpoLdsBytes);
  if (err == hipSuccess) err = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_net_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kPpoLdsBytes);
  return err;
}

void ppo_launch(const PpoLaunch& a, hipStream_t s) {
  const int64_t groups = ppo_workgroups(a.n);
  float* parts = a.workspace + 2 * kPpoBwdFloats;
  hipLaunchKernelGGL(ppo_transpose_kernel, dim3(kPpoBwdFrags + 1, 2), dim3(512), 0, s, a.actor_block, a.critic_block, a.workspace);
  PpoNetArgs net = {a.actor_block, a.workspace, a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, a.indices, a.n,
                    a.clip_lo, a.clip_hi, a.clip_range, 2.0f * a.vf_coef, parts, a.log_prob};
  hipLaunchKernelGGL((ppo_net_kernel<true, false>), dim3((unsigned)groups), dim3(kPolBlock), kPpoLdsBytes, s, net);
  net.block = a.critic_block; net.bwd = a.workspace + kPpoBwdFloats; net.out = a.values;
  hipLaunchKernelGGL((ppo_net_kernel<false, false>), dim3((unsigned)groups), dim3(kPolBlock), kPpoLdsBytes, s, net);
  const int total = kPpoActorGrad + kPpoCriticGrad + 1;
  hipLaunchKernelGGL(ppo_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s, parts, groups, a.n, a.actor_block, a.ent_coef, a.vf_coef,
                     a.actor_grad, a.critic_grad, a.scalars);
}

void ppo_set_launch(const PpoSetLaunch& L, hipStream_t s) {
  const PpoLaunch& a = L.a;
  const unsigned P = (unsigned)L.n_members;
  hipLaunchKernelGGL(ppo_set_transpose_kernel, dim3(kPpoBwdFrags + 1, 2, P), dim3(512), 0, s, a.actor_block, a.critic_block, a.workspace, L.table);
  PpoSetNetArgs S = {{a.actor_block, nullptr, a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, a.indices, 0,
                      a.clip_lo, a.clip_hi, a.clip_range, 2.0f * a.vf_coef, a.workspace, a.log_prob}, L.table};
  hipLaunchKernelGGL((ppo_net_kernel<true, true>), dim3((unsigned)L.max_workgroups, P), dim3(kPolBlock), kPpoLdsBytes, s, S);
  S.net.block = a.critic_block; S.net.out = a.values;
  hipLaunchKernelGGL((ppo_net_kernel<false, true>), dim3((unsigned)L.max_workgroups, P), dim3(kPolBlock), kPpoLdsBytes, s, S);
  const int total = kPpoActorGrad + kPpoCriticGrad + 1;
  hipLaunchKernelGGL(ppo_set_finish_kernel, dim3((total + 255) / 256, P), dim3(256), 0, s, a.workspace, a.actor_block, a.ent_coef, a.vf_coef,
                     a.actor_grad, a.critic_grad, a.scalars, L.table);
}

}  // namespace rdv

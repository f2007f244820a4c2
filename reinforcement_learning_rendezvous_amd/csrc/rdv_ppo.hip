// rdv_ppo.hip — the kernels of rdv_ppo.h and their launch, in a translation unit of its own (the objects of the other units do not change
// when it does).  The exported rdv_ppo_* entry points are in rdv_policy_host.hip, with the other policy entry points.  This unit holds the
// shipped architecture's own: its three layers, its forward pass with the activations kept, the set form, the launches.  The gather, the
// loss terms, the weight-gradient contraction and the other pieces it has in common with rdv_ppo_mlp.hip are the functions of rdv_ppo_ops.h.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_ppo.h"
#include "rdv_ppo_ops.h"

#include <type_traits>

namespace rdv {

// LDS of ppo_net_kernel (floats): parameters | per wave: observation rows [32][17] | per wave: three operand tiles | per wave: 4 scalar sums
// (the tiles and a wave's share: rdv_ppo_ops.h)
constexpr int kPpoWaves = kPolBlock / 64;
constexpr int kPpoLdsObs = kPolFloats, kPpoLdsTiles = kPpoLdsObs + kPpoWaves * kPolObsStage, kPpoLdsRed = kPpoLdsTiles + kPpoWaves * kPpoWaveTiles;
constexpr int kPpoLdsBytes = (kPolFloats + kPpoWaves * kPpoWaveFloats) * 4;   // 149,328 B: one workgroup per CU
static_assert(kPpoLdsBytes == (kPpoLdsRed + kPpoWaves * 4) * 4 && kPpoLdsBytes <= 160 * 1024, "the workgroup's LDS");
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
  const PpoTransposeIndex x = ppo_transpose_index(ks, h, j, mt, r);
  const int frag = head ? kPolW3Frag + q * 4 + x.ks_i : kPolW2Frag + (q * 2 + (x.o >> 5)) * 4 + x.ks_i;
  reinterpret_cast<uint16_t*>(dstf)[(b * 64 + lane) * 8 + j] = src[(frag * 64 + (x.o & 31) + 32 * x.h_i) * 8 + x.j_i];
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
  PpoRowArgs rows;
  float* parts;                  // [workgroups][kPpoPartFloats]
  float* out;                    // nullable [n]: log_prob (actor) or values (critic)
};

// actor_means of rdv_policy.h with the hidden activations kept: hs1, hs2 [row tile][accumulator register], times 2^10
__device__ __forceinline__ void ppo_forward(const float* w, const float* rows, int lane, float (&hs1)[2][16], float (&hs2)[2][16], float (&mean)[4]) {
  f16x8 x0[2][2];
  actor_inputs(rows, lane, x0);
  constexpr float two_log2e = 2.8853900817779268f;
  f32x16 d1[2];
  layer<2, 2>(w, kPolW1Frag, w + kPolB1, x0, lane, d1);
  f16x8 x1[4][2];
  const float k1 = two_log2e * w[kPolScale + 0];
  ppo_activate_keep<RDV_ACT_TANH>(d1[0], k1, x1[0], x1[1], hs1[0]);
  ppo_activate_keep<RDV_ACT_TANH>(d1[1], k1, x1[2], x1[3], hs1[1]);
  f32x16 d2[2];
  layer<2, 4>(w, kPolW2Frag, w + kPolB2, x1, lane, d2);
  f16x8 x2[4][2];
  const float k2 = two_log2e * w[kPolScale + 1];
  ppo_activate_keep<RDV_ACT_TANH>(d2[0], k2, x2[0], x2[1], hs2[0]);
  ppo_activate_keep<RDV_ACT_TANH>(d2[1], k2, x2[2], x2[3], hs2[1]);
  f32x16 d3[1];
  layer<1, 4>(w, kPolW3Frag, w + kPolB3, x2, lane, d3);
  const float s3 = w[kPolScale + 2];
  mean[0] = d3[0][0] * s3; mean[1] = d3[0][1] * s3; mean[2] = d3[0][2] * s3; mean[3] = d3[0][3] * s3;
}

// delta = pre o (1 - h^2) * unscale for one tile (hs = h * 2^10)
__device__ __forceinline__ void error_tile(const f32x16& pre, const float (&hs)[16], float unscale, float (&delta)[16]) {
  constexpr float inv = 1.0f / (float)(1 << kPolXShift);
#pragma unroll
  for (int e = 0; e < 16; ++e) { const float hv = hs[e] * inv; delta[e] = pre[e] * (1.0f - hv * hv) * unscale; }
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
    M.rows.indices = S.net.rows.indices + off;
    M.rows.n = n;
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
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31;
  float* rows = lds + kPpoLdsObs + wv * kPolObsStage;
  float* tiles0 = lds + kPpoLdsTiles;
  float* wave_tiles = tiles0 + wv * kPpoWaveTiles;
  float* red = lds + kPpoLdsRed;
  const int64_t wave_base = ((int64_t)blockIdx.x * kPpoWaves + wv) * kPolWaveEnvs;
  const int64_t left = A.rows.n - wave_base;
  const int nrows = left < 0 ? 0 : (left < kPolWaveEnvs ? (int)left : kPolWaveEnvs);   // trailing waves: 0 rows, and they stay (barriers below)

  for (int q = threadIdx.x; q < kPolFloats / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(A.block + 4 * q);

  bool valid;
  const int64_t src = ppo_gather_rows(A.rows, wave_base, nrows, rows, lane, valid);
  __syncthreads();

  float hs1[2][16], hs2[2][16], mean[4];
  ppo_forward(w, rows, lane, hs1, hs2, mean);

  float d3[4], ex[4];
  ppo_loss_terms<ACTOR>(A.rows, w + kPolStd, w + kPolLogStd, mean, valid, src, A.out, wave_base + r, lane, red + wv * 4, d3, ex);

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
    weight_grads<1, 2, kPpoWaves>(head, wave_tiles, tiles0, 0, invS3 * inv_xs, lane, [&](int row, int col, float v) {
      if (col >= 0) { if (row < OUT) part[kPpoW3 + row * kPolHid + col] = v; }
      else if (col == -1) {
        if (row < OUT) part[kPpoW3 + OUT * kPolHid + row] = v;
        if (ACTOR && row >= 8 && row < 8 + kPolOut) part[kPpoW3 + OUT * kPolHid + OUT + (row - 8)] = v;
      }
    });
  }
  // the workgroup's scalar sums (red[] is behind a barrier by now)
  ppo_store_scalar_sums<ACTOR>(red, kPpoWaves, A.parts + (size_t)blockIdx.x * kPpoPartFloats + kPpoPartScalars);

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
#pragma unroll
    for (int s = 0; s < 4; ++s) error_frags(delta2[s >> 1], s & 1, b2[s]);
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
    weight_grads<2, 2, kPpoWaves>(delta2, wave_tiles, tiles0, 0, invS2 * inv_xs, lane, [&](int row, int col, float v) {
      if (col >= 0) part[kPpoW2 + row * kPolHid + col] = v;
      else if (col == -1) part[kPpoB2 + row] = v;
    });
  }

  // ---- layer 1: dW1 = delta_1 . x^T with the staged observation rows as the forward pass reads them (times 2^10, clamped to +-63), db1
  float S1, invS1;
  wave_scale(fmaxf(tile_max(delta1[0]), tile_max(delta1[1])), S1, invS1);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) delta1[mt][e] *= S1;
  float xin[16];
  ppo_input_tile(rows, lane, xin);
  stage_tile(reinterpret_cast<_Float16*>(wave_tiles), xin, lane);
  weight_grads<2, 1, kPpoWaves>(delta1, wave_tiles, tiles0, 0, invS1 * inv_xs, lane, [&](int row, int col, float v) {
    if (col >= 0) { if (col < kPolIn) part[kPpoW1 + row * kPolIn + col] = v; }
    else if (col == -1) part[kPpoB1 + row] = v;
  });
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
    ppo_finish_scalars(s, n, actor_block + kPolLogStd, ent_coef, vf_coef, scalars);
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
  PpoNetArgs net = {a.actor_block, a.workspace, ppo_row_args(a), parts, a.log_prob};
  hipLaunchKernelGGL((ppo_net_kernel<true, false>), dim3((unsigned)groups), dim3(kPolBlock), kPpoLdsBytes, s, net);
  net.block = a.critic_block; net.bwd = a.workspace + kPpoBwdFloats; net.out = a.values;
  hipLaunchKernelGGL((ppo_net_kernel<false, false>), dim3((unsigned)groups), dim3(kPolBlock), kPpoLdsBytes, s, net);
  const int total = kPpoActorGrad + kPpoCriticGrad + 1;
  hipLaunchKernelGGL(ppo_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s, parts, groups, a.n, a.actor_block, a.k.ent_coef, a.k.vf_coef,
                     a.actor_grad, a.critic_grad, a.scalars);
}

void ppo_set_launch(const PpoSetLaunch& L, hipStream_t s) {
  const PpoLaunch& a = L.a;
  const unsigned P = (unsigned)L.n_members;
  hipLaunchKernelGGL(ppo_set_transpose_kernel, dim3(kPpoBwdFrags + 1, 2, P), dim3(512), 0, s, a.actor_block, a.critic_block, a.workspace, L.table);
  PpoSetNetArgs S = {{a.actor_block, nullptr, ppo_row_args(a), a.workspace, a.log_prob}, L.table};   // a.n is 0: the members' counts are the table's
  hipLaunchKernelGGL((ppo_net_kernel<true, true>), dim3((unsigned)L.max_workgroups, P), dim3(kPolBlock), kPpoLdsBytes, s, S);
  S.net.block = a.critic_block; S.net.out = a.values;
  hipLaunchKernelGGL((ppo_net_kernel<false, true>), dim3((unsigned)L.max_workgroups, P), dim3(kPolBlock), kPpoLdsBytes, s, S);
  const int total = kPpoActorGrad + kPpoCriticGrad + 1;
  hipLaunchKernelGGL(ppo_set_finish_kernel, dim3((total + 255) / 256, P), dim3(256), 0, s, a.workspace, a.actor_block, a.k.ent_coef, a.k.vf_coef,
                     a.actor_grad, a.critic_grad, a.scalars, L.table);
}

}  // namespace rdv

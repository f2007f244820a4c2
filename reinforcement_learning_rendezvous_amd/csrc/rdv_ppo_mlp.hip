// rdv_ppo_mlp.hip — the kernels of rdv_ppo_mlp.h and their launch, in a translation unit of its own (the objects of the other units do
// not change when it does).  The exported rdv_ppo_mlp_* entry points are in rdv_policy_host.hip, with the other policy entry points.
// This unit holds what a table of layers needs: the transposed fragments, the recomputed forward pass, one backward step per (tiles,
// k-steps) shape, the launches.  The gather, the loss terms, the weight-gradient contraction and the other pieces it has in common with
// rdv_ppo.hip are the functions of rdv_ppo_ops.h.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_ppo_mlp.h"

#include <type_traits>

namespace rdv {

// LDS of ppo_mlp_net_kernel (floats), W = waves of the workgroup (8 or 4, ppo_mlp_waves):
//   parameter block | per wave: observation rows [32][17] | per wave: three operand tiles | per wave: 4 scalar sums
// (the tiles and a wave's share: rdv_ppo_ops.h)
static_assert((kMlpMaxFloats + 4 * kPpoWaveFloats) * 4 <= kPpoMlpLdsLimit, "the largest block with four waves fits the CU's LDS");

// ---- 1. the transposed fragments of one net.  Backward fragment (q, mt, ks) of layer l, lane (r, h), element j:
//   W_l,q[o][i],  o = perm(ks, h, j) (the k order of an accumulator tile used as B operand),  i = 32 mt + r,
// read from where the forward block keeps it: fragment frag0_l + (q MT_l + (o >> 5)) KS_l + ks(i), lane (o & 31, h(i)), element j(i) — the
// inverse of perm — or zero where the forward layer has no such tile row or k-step (a 16-wide neighbour).
__device__ __forceinline__ void ppo_mlp_transpose_body(const float* __restrict__ block, float* __restrict__ dstf) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b == kPpoMlpBwdFrags) { if (t < 64) dstf[kPpoMlpBwdZero + t] = 0.0f; return; }
  const int32_t* H = reinterpret_cast<const int32_t*>(block);
  const int L = H[0];
  int l = 0, base = 0, MTh = 1, KSd = 1;
  for (int k = 1, at = 0; k <= L; ++k) {
    const int mth = H[kMlpRec + kMlpRecStride * (k - 1) + 2], ksd = k < L ? H[kMlpRec + kMlpRecStride * (k + 1) + 3] : 1;
    const int count = 2 * mth * ksd;
    if (b >= at && b < at + count) { l = k; base = at; MTh = mth; KSd = ksd; }
    at += count;
  }
  if (l == 0) return;                                     // a fragment slot this architecture does not use
  const int32_t* rec = H + kMlpRec + kMlpRecStride * l;
  const int frag0 = rec[0], MT = rec[2], KS = rec[3];
  const int bb = b - base, q = bb / (MTh * KSd), mt = (bb / KSd) % MTh, ks = bb % KSd;
  const int lane = t >> 3, j = t & 7, r = lane & 31, h = lane >> 5;
  const PpoTransposeIndex x = ppo_transpose_index(ks, h, j, mt, r);
  uint16_t v = 0;
  if ((x.o >> 5) < MT && x.ks_i < KS) {
    const uint16_t* src = reinterpret_cast<const uint16_t*>(block + kMlpHdr);
    v = src[((size_t)(frag0 + (q * MT + (x.o >> 5)) * KS + x.ks_i) * 64 + (size_t)((x.o & 31) + 32 * x.h_i)) * 8 + x.j_i];
  }
  reinterpret_cast<uint16_t*>(dstf)[((size_t)b * 64 + lane) * 8 + j] = v;
}
__global__ __launch_bounds__(512) void ppo_mlp_transpose_kernel(const float* __restrict__ actor_block, const float* __restrict__ critic_block,
                                                                float* __restrict__ workspace) {
  ppo_mlp_transpose_body(blockIdx.y == 0 ? actor_block : critic_block, workspace + (size_t)blockIdx.y * kPpoMlpBwdFloats);
}
// the set form: member blockIdx.z of the sets' allocations -> the head of its piece of the workspace; a member without samples is skipped
__global__ __launch_bounds__(512) void ppo_mlp_set_transpose_kernel(const float* __restrict__ actor_set, const float* __restrict__ critic_set,
                                                                    float* __restrict__ workspace, int actor_floats, int critic_floats,
                                                                    const PpoSetTable T) {
  const int g = blockIdx.z;
  if (T.count[g] == 0) return;
  const float* block = blockIdx.y == 0 ? actor_set + (size_t)g * actor_floats : critic_set + (size_t)g * critic_floats;
  ppo_mlp_transpose_body(block, workspace + T.ws[g] + (size_t)blockIdx.y * kPpoMlpBwdFloats);
}

// ---- 2, 3. one net's loss terms and gradients
struct PpoMlpNetArgs {
  const float *block, *bwd;      // forward parameter block, backward block (workspace)
  PpoRowArgs rows;
  float* parts;                  // [workgroups][T.part_floats]
  float* out;                    // nullable [n]: log_prob (actor) or values (critic)
  PpoMlpTable T;
};

// layer 0: dW_0 = delta_0 . x^T with the staged observation rows as the forward pass reads them (times 2^10, clamped to +-63), db_0
template <int MTd>
__device__ __forceinline__ void input_step(const PpoMlpTable& T, float (&dl)[2][16], const float* rows, float* wave_tiles, const float* tiles0, int nw,
                                           int lane, float* part) {
  constexpr float inv_xs = 1.0f / (float)(1 << kPolXShift);
  float S, invS;
  wave_scale(MTd == 2 ? fmaxf(tile_max(dl[0]), tile_max(dl[1])) : tile_max(dl[0]), S, invS);
#pragma unroll
  for (int mt = 0; mt < MTd; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dl[mt][e] *= S;
  float xin[16];
  ppo_input_tile(rows, lane, xin);
  stage_tile(reinterpret_cast<_Float16*>(wave_tiles), xin, lane);
  const int w_off = T.w_off[0], b_off = T.b_off[0], out_w = T.out_w[0];
  weight_grads<MTd, 1, 0>(dl, wave_tiles, tiles0, nw, invS * inv_xs, lane, [&](int row, int col, float v) {
    if (col >= 0) { if (row < out_w && col < kPolIn) part[w_off + row * kPolIn + col] = v; }
    else if (col == -1 && row < out_w) part[b_off + row] = v;
  });
}

// The set form's arguments: `net` holds the set-wide values (block: the set's allocation; parts: the workspace; rows.indices and out: all
// members'; bwd and rows.n unused; T: the one table of this net); ppo_mlp_member derives member blockIdx.y's own WITHOUT the table, which
// stays in the kernel-argument segment (a private copy indexed by the layer would be scratch).  skip_shift, skip_part: a critic's rows of
// partial sums lie behind the actor's, ((n + 2^skip_shift - 1) >> skip_shift) rows of skip_part floats.  `idle`: workgroup x has no rows
// of that member (it has fewer workgroups than the widest member, or no samples) — workgroup-uniform, taken before the first barrier.
struct PpoMlpSetNetArgs {
  PpoMlpNetArgs net;
  int32_t skip_shift, skip_part;
  PpoSetTable table;
};
static_assert(sizeof(PpoMlpSetNetArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
struct PpoMlpMember {
  const float *block, *bwd;
  PpoRowArgs rows;
  float *parts, *out;
};
template <bool SET> using PpoMlpKernelArgs = std::conditional_t<SET, PpoMlpSetNetArgs, PpoMlpNetArgs>;
__host__ __device__ __forceinline__ const PpoMlpTable& ppo_mlp_table_of(const PpoMlpNetArgs& S) { return S.T; }
__host__ __device__ __forceinline__ const PpoMlpTable& ppo_mlp_table_of(const PpoMlpSetNetArgs& S) { return S.net.T; }
template <bool ACTOR, bool SET>
__device__ __forceinline__ decltype(auto) ppo_mlp_member(const PpoMlpKernelArgs<SET>& S, bool& idle) {
  if constexpr (SET) {
    const int g = blockIdx.y;
    const int64_t n = S.table.count[g], off = S.table.off[g];
    idle = (int64_t)blockIdx.x * (S.net.T.waves * kPolWaveEnvs) >= n;
    float* ws = S.net.parts + S.table.ws[g];
    PpoMlpMember M;
    M.block = S.net.block + (size_t)g * S.net.T.block_floats;
    M.bwd = ws + (ACTOR ? 0 : kPpoMlpBwdFloats);
    M.rows = S.net.rows;
    M.rows.indices = S.net.rows.indices + off;
    M.rows.n = n;
    M.parts = ws + 2 * kPpoMlpBwdFloats + (ACTOR ? (int64_t)0 : ((n + ((int64_t)1 << S.skip_shift) - 1) >> S.skip_shift) * S.skip_part);
    M.out = S.net.out ? S.net.out + off : nullptr;
    return M;
  } else {
    idle = false;
    return (S);                                            // the arguments themselves: the plain kernel is the code it was
  }
}
// The workgroup has blockDim.x / 64 waves (T.waves), each 32 rows; trailing waves of the last workgroup have no rows and stay (barriers).
// SET = false: the kernel of rdv_ppo_mlp_loss_grad (profiles/ppo_mlp_set_isa_diff.md).  SET = true: workgroup (x, y) is workgroup x of
// member y's stand-alone launch: the same body on the member's arguments.
template <int ACT, bool ACTOR, bool SET>
__global__ __launch_bounds__(kPolBlock) void ppo_mlp_net_kernel(const PpoMlpKernelArgs<SET> S) {
  bool idle;
  const auto& A = ppo_mlp_member<ACTOR, SET>(S, idle);
  if (SET && idle) return;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const PpoMlpTable& T = ppo_mlp_table_of(S);
  const int32_t* H = reinterpret_cast<const int32_t*>(A.block);
  const int total = T.block_floats, L = T.L, nw = T.waves;
  float* w = lds;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31;
  float* rows = lds + total + wv * kPolObsStage;
  float* tiles0 = lds + total + nw * kPolObsStage;
  float* wave_tiles = tiles0 + wv * kPpoWaveTiles;
  float* red = tiles0 + nw * kPpoWaveTiles;
  const int64_t wave_base = ((int64_t)blockIdx.x * nw + wv) * kPolWaveEnvs;
  const int64_t left = A.rows.n - wave_base;
  const int nrows = left < 0 ? 0 : (left < kPolWaveEnvs ? (int)left : kPolWaveEnvs);

  for (int q = threadIdx.x; q < total / 4; q += nw * 64)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(A.block + 4 * q);

  bool valid;
  const int64_t src = ppo_gather_rows(A.rows, wave_base, nrows, rows, lane, valid);
  __syncthreads();

  float* part = A.parts + (size_t)blockIdx.x * T.part_floats;
  f16x8 x[4][2];
  float hs[2][16], dl[2][16];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) { hs[mt][e] = 0.0f; dl[mt][e] = 0.0f; }

#pragma nounroll
  for (int l = L; l >= 1; --l) {
    mlp_forward_keep<ACT>(w, H, rows, lane, l, x, hs);     // h_l, recomputed: the forward's own operations
    const int32_t* rec = H + kMlpRec + kMlpRecStride * l;
    if (l == L) {
      // ---- the head and the loss terms of this lane's row: the head's error (times n) in registers 0..3 of the tile, the d log_std terms
      // in registers 4..7 (actor), the scalar sums
      float mean[4];
      {
        const float* wf = w + kMlpHdr;
        const float* zerop = w + kMlpZero;
        const float* biasp = w + rec[1];
        const float inv = __int_as_float(rec[4]);
        switch (rec[3]) {
          case 1: mlp_head<1>(wf, zerop, rec[0], biasp, inv, lane, x, mean); break;
          case 2: mlp_head<2>(wf, zerop, rec[0], biasp, inv, lane, x, mean); break;
          default: mlp_head<4>(wf, zerop, rec[0], biasp, inv, lane, x, mean); break;
        }
      }
      float d3[4], ex[4];
      ppo_loss_terms<ACTOR>(A.rows, w + kMlpStd, w + kMlpStd + 8, mean, valid, src, A.out, wave_base + r, lane, red + wv * 4, d3, ex);
#pragma unroll
      for (int c = 0; c < 4; ++c) { dl[0][c] = d3[c]; dl[0][4 + c] = ex[c]; }   // features 4 h + c, and 8 + 4 h + c
    }
    const float inv_acc = __int_as_float(rec[4]);
    const int MTh = T.mt[l - 1], KSd = l < L ? T.ks[l + 1] : 1;
    switch (MTh * 8 + KSd) {
      case 8 + 1: backward_step<ACT, ACTOR, 1, 1>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
      case 8 + 2: backward_step<ACT, ACTOR, 1, 2>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
      case 8 + 4: backward_step<ACT, ACTOR, 1, 4>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
      case 16 + 1: backward_step<ACT, ACTOR, 2, 1>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
      case 16 + 2: backward_step<ACT, ACTOR, 2, 2>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
      default: backward_step<ACT, ACTOR, 2, 4>(T, l, A.bwd, inv_acc, dl, hs, wave_tiles, tiles0, nw, lane, part); break;
    }
    if (l == L) ppo_store_scalar_sums<ACTOR>(red, nw, part + T.part_floats - 4);   // red[] is behind a barrier by now
  }
  if (T.mt[0] == 2) input_step<2>(T, dl, rows, wave_tiles, tiles0, nw, lane, part);
  else input_step<1>(T, dl, rows, wave_tiles, tiles0, nw, lane, part);
}

// ---- 4. the workgroups' rows added in index order -> the gradients (divided by n; - ent_coef on d log_std) and the scalars
struct PpoMlpFinishArgs {
  const float *actor_parts, *critic_parts;
  int64_t actor_groups, critic_groups, n;
  int32_t actor_stride, critic_stride, actor_floats, critic_floats;
  const float* actor_block;
  float ent_coef, vf_coef;
  float *actor_grad, *critic_grad, *scalars;
};
__device__ __forceinline__ void ppo_mlp_finish_body(const PpoMlpFinishArgs& F) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float fn = (float)F.n;
  if (i < F.actor_floats) {
    float sum = 0.0f;
    for (int64_t g = 0; g < F.actor_groups; ++g) sum += F.actor_parts[g * F.actor_stride + i];
    float v = sum / fn;
    if (i >= F.actor_floats - kPolOut) v -= F.ent_coef;
    F.actor_grad[i] = v;
  } else if (i < F.actor_floats + F.critic_floats) {
    const int k = i - F.actor_floats;
    float sum = 0.0f;
    for (int64_t g = 0; g < F.critic_groups; ++g) sum += F.critic_parts[g * F.critic_stride + k];
    F.critic_grad[k] = sum / fn;
  } else if (i == F.actor_floats + F.critic_floats) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t g = 0; g < F.actor_groups; ++g)
      for (int k = 0; k < 3; ++k) s[k] += (double)F.actor_parts[g * F.actor_stride + F.actor_stride - 4 + k];
    for (int64_t g = 0; g < F.critic_groups; ++g) s[3] += (double)F.critic_parts[g * F.critic_stride + F.critic_stride - 1];
    ppo_finish_scalars(s, F.n, F.actor_block + kMlpStd + 8, F.ent_coef, F.vf_coef, F.scalars);
  }
}

__global__ __launch_bounds__(256) void ppo_mlp_finish_kernel(const PpoMlpFinishArgs F) { ppo_mlp_finish_body(F); }
// the set form: member blockIdx.y's rows of the workspace -> row blockIdx.y of the outputs; nothing of a member without samples is
// written.  `F` holds the set-wide values (actor_parts: the workspace; actor_block: the actor set's allocation; the outputs' row 0;
// critic_parts, the group counts and n unused).
struct PpoMlpSetFinishArgs {
  PpoMlpFinishArgs F;
  int32_t actor_shift, critic_shift, block_floats;     // rows per workgroup of either net as a shift; the actor's block
  PpoSetTable table;
};
static_assert(sizeof(PpoMlpSetFinishArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
__global__ __launch_bounds__(256) void ppo_mlp_set_finish_kernel(const PpoMlpSetFinishArgs S) {
  const int g = blockIdx.y;
  const int64_t n = S.table.count[g];
  if (n == 0) return;
  PpoMlpFinishArgs F = S.F;
  F.n = n;
  F.actor_groups = (n + ((int64_t)1 << S.actor_shift) - 1) >> S.actor_shift;
  F.critic_groups = (n + ((int64_t)1 << S.critic_shift) - 1) >> S.critic_shift;
  F.actor_parts = S.F.actor_parts + S.table.ws[g] + 2 * kPpoMlpBwdFloats;
  F.critic_parts = F.actor_parts + F.actor_groups * F.actor_stride;
  F.actor_block = S.F.actor_block + (size_t)g * S.block_floats;
  F.actor_grad = S.F.actor_grad + (size_t)g * F.actor_floats;
  F.critic_grad = S.F.critic_grad + (size_t)g * F.critic_floats;
  F.scalars = S.F.scalars + (size_t)g * kPpoScalars;
  ppo_mlp_finish_body(F);
}

template <bool ACTOR, bool SET>
static const void* net_kernel_of(int activation) {
  switch (activation) {
    case RDV_ACT_RELU: return reinterpret_cast<const void*>(ppo_mlp_net_kernel<RDV_ACT_RELU, ACTOR, SET>);
    case RDV_ACT_SIGMOID: return reinterpret_cast<const void*>(ppo_mlp_net_kernel<RDV_ACT_SIGMOID, ACTOR, SET>);
    default: return reinterpret_cast<const void*>(ppo_mlp_net_kernel<RDV_ACT_TANH, ACTOR, SET>);
  }
}

hipError_t ppo_mlp_raise_lds_limit() {
  for (int act = 0; act < 3; ++act) {
    const void* kernels[] = {net_kernel_of<true, false>(act), net_kernel_of<false, false>(act), net_kernel_of<true, true>(act), net_kernel_of<false, true>(act)};
    for (const void* k : kernels) {
      hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kPpoMlpLdsLimit);
      if (err != hipSuccess) return err;
    }
  }
  return hipSuccess;
}

template <bool ACTOR, bool SET>
static void launch_net(int activation, const PpoMlpKernelArgs<SET>& net, dim3 grid, hipStream_t s) {
  const PpoMlpTable& T = ppo_mlp_table_of(net);
  const dim3 block((unsigned)(T.waves * 64));
  const int lds = ppo_mlp_lds_bytes(T);
  switch (activation) {
    case RDV_ACT_RELU: hipLaunchKernelGGL((ppo_mlp_net_kernel<RDV_ACT_RELU, ACTOR, SET>), grid, block, lds, s, net); break;
    case RDV_ACT_SIGMOID: hipLaunchKernelGGL((ppo_mlp_net_kernel<RDV_ACT_SIGMOID, ACTOR, SET>), grid, block, lds, s, net); break;
    default: hipLaunchKernelGGL((ppo_mlp_net_kernel<RDV_ACT_TANH, ACTOR, SET>), grid, block, lds, s, net); break;
  }
}

void ppo_mlp_launch_transpose(const float* actor_block, const float* critic_block, float* workspace, hipStream_t s) {
  hipLaunchKernelGGL(ppo_mlp_transpose_kernel, dim3(kPpoMlpBwdFrags + 1, 2), dim3(512), 0, s, actor_block, critic_block, workspace);
}

void ppo_mlp_launch_set_transpose(const float* actor_set, const float* critic_set, float* workspace, int actor_floats, int critic_floats, int32_t n_members,
                                  const PpoSetTable& table, hipStream_t s) {
  hipLaunchKernelGGL(ppo_mlp_set_transpose_kernel, dim3(kPpoMlpBwdFrags + 1, 2, (unsigned)n_members), dim3(512), 0, s, actor_set, critic_set, workspace,
                     actor_floats, critic_floats, table);
}

void ppo_mlp_launch(const PpoMlpLaunch& a, hipStream_t s) {
  const int64_t groups_a = ppo_mlp_workgroups(a.actor, a.n), groups_c = ppo_mlp_workgroups(a.critic, a.n);
  float* parts_a = a.workspace + 2 * kPpoMlpBwdFloats;
  float* parts_c = parts_a + groups_a * a.actor.part_floats;
  hipLaunchKernelGGL(ppo_mlp_transpose_kernel, dim3(kPpoMlpBwdFrags + 1, 2), dim3(512), 0, s, a.actor_block, a.critic_block, a.workspace);
  PpoMlpNetArgs net = {a.actor_block, a.workspace, ppo_row_args(a), parts_a, a.log_prob, a.actor};
  launch_net<true, false>(a.actor_act, net, dim3((unsigned)groups_a), s);
  net.block = a.critic_block; net.bwd = a.workspace + kPpoMlpBwdFloats; net.parts = parts_c; net.out = a.values; net.T = a.critic;
  launch_net<false, false>(a.critic_act, net, dim3((unsigned)groups_c), s);
  const PpoMlpFinishArgs F = {parts_a, parts_c, groups_a, groups_c, a.n, a.actor.part_floats, a.critic.part_floats, a.actor.grad_floats,
                              a.critic.grad_floats, a.actor_block, a.k.ent_coef, a.k.vf_coef, a.actor_grad, a.critic_grad, a.scalars};
  const int total = a.actor.grad_floats + a.critic.grad_floats + 1;
  hipLaunchKernelGGL(ppo_mlp_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s, F);
}

// rows per workgroup (256 or 128) as a shift
static int rows_shift(const PpoMlpTable& t) { return t.waves == 8 ? 8 : 7; }

void ppo_mlp_set_launch(const PpoMlpSetLaunch& L, hipStream_t s) {
  const PpoMlpLaunch& a = L.a;
  const unsigned P = (unsigned)L.n_members;
  ppo_mlp_launch_set_transpose(a.actor_block, a.critic_block, a.workspace, a.actor.block_floats, a.critic.block_floats, L.n_members, L.table, s);
  PpoMlpSetNetArgs S = {{a.actor_block, nullptr, ppo_row_args(a), a.workspace, a.log_prob, a.actor}, 0, 0, L.table};   // a.n is 0: the counts are the table's
  launch_net<true, true>(a.actor_act, S, dim3((unsigned)L.max_groups_a, P), s);
  S.net.block = a.critic_block; S.net.out = a.values; S.net.T = a.critic;
  S.skip_shift = rows_shift(a.actor); S.skip_part = a.actor.part_floats;
  launch_net<false, true>(a.critic_act, S, dim3((unsigned)L.max_groups_c, P), s);
  const PpoMlpSetFinishArgs F = {{a.workspace, nullptr, 0, 0, 0, a.actor.part_floats, a.critic.part_floats, a.actor.grad_floats, a.critic.grad_floats,
                                  a.actor_block, a.k.ent_coef, a.k.vf_coef, a.actor_grad, a.critic_grad, a.scalars},
                                 rows_shift(a.actor), rows_shift(a.critic), a.actor.block_floats, L.table};
  const int total = a.actor.grad_floats + a.critic.grad_floats + 1;
  hipLaunchKernelGGL(ppo_mlp_set_finish_kernel, dim3((total + 255) / 256, P), dim3(256), 0, s, F);
}

}  // namespace rdv

// rdv_ppo_mlp.h — the PPO minibatch loss and its gradients (rdv_ppo.h) for every architecture of rdv_policy_mlp.h: 1..4 hidden layers of
// 16 / 32 / 64, tanh / ReLU / sigmoid, actor and critic each of a spec of its own (rdv_ppo_mlp_loss_grad, include/rdv.h "PPO minibatch
// gradients for every MLP architecture").  The kernels are in rdv_ppo_mlp.hip, a translation unit of its own; this header holds the sizes,
// the layer table and the launch that the host unit (rdv_policy_host.hip) needs, and the description.  The scheme is rdv_ppo.h's: the
// same four launches, the same operands (wave-scaled error tiles split into two fp16 terms, mfma3, the LDS operand tiles of dW), the same
// sums (waves in order, workgroups in index order); what changes is that the layers are a table and not three lines of code.  Everything
// else — the row arguments, a wave's LDS share, the gather, the loss terms, the kept activation, the weight-gradient contraction, the
// tail of the last kernel — is defined once, in rdv_ppo_ops.h, for this unit and rdv_ppo.hip.
//
//   1. ppo_mlp_transpose_kernel: for layers l = 1 .. L (L: the head) the A-operand fragments of W_l^T, derived from the handle's FORWARD
//      block through its layer table (first fragment, MT, KS per layer) into the head of the workspace.  Fragment (q, mt, ks) of layer l,
//      lane (r, h), element j holds W_l,q[perm(ks, h, j)][32 mt + r]; mt runs over the tiles of the layer's INPUT (h_l), ks over the
//      k-steps of its OUTPUT (delta_l; the head: one).  A 16-wide input has rows 16..31 of its one tile and a 16-wide output its missing
//      k-steps as ZERO fragments: the forward block holds no such weights.
//   2, 3. ppo_mlp_net_kernel<ACT, ACTOR> (six instantiations, as mlp_kernel): a wave owns 32 minibatch rows.  Per wave: gather the rows,
//      then ONE loop over the layers from the head down, its body a wave-uniform switch over the six (tiles of h_l, k-steps of delta_l)
//      shapes: delta_{l-1} = (W_l^T delta_l) o act'(h_l), dW_l = delta_l h_l^T and db_l through the LDS operand tiles; layer 0 contracts
//      with the observation rows as the forward pass reads them (clamped to +-63).  The workgroup's sums go to its row of the workspace.
//   4. ppo_mlp_finish_kernel: the workgroups' rows added in index order, over the two specs' gradient lengths.
//
// Two decisions:
//   Kept activations: RECOMPUTED.  The backward step of layer l needs h_l alone (for act' and as the B operand of dW_l), so the loop
//      runs the forward pass up to layer l — the device functions of rdv_policy_mlp.h, with the activation kept in accumulator order —
//      in front of each step: L (L + 1) / 2 hidden layers per wave instead of L, 10 instead of 4 for four layers.  A forward layer is
//      at most 24 MFMAs and no barrier; a backward step is as many plus the dW tiles with two barriers each, so the forward share stays
//      small, no activation lives across a step (registers: x, one layer's h, one error tile set), and the LDS per wave stays the
//      14,480 B of rdv_ppo.hip (observation rows, three operand tiles, four sums) whatever the depth.  Keeping four layers in registers
//      would need dynamic indexing (scratch) or a fully unrolled loop per architecture; keeping them in LDS 8 KiB per layer and wave.
//   LDS: the forward block is RESIDENT, as in the forward kernels, and the workgroup has EIGHT waves (256 rows) where block + 8 x 14,480 B
//      fit the CU's 160 KiB — blocks up to 48,000 B: [64, 64] 33,920 B, [64, 64, 32] 38,144 B, 4 x 32 and everything narrower —
//      and FOUR waves (128 rows, 256 threads) otherwise ([64, 64, 64]: 50,560 B; 4 x 64: 67,200 + 57,920 = 125,120 B).  ppo_mlp_waves is a function of the net's
//      spec alone, so the partition of the minibatch into workgroups, and with it every bit of the sums, depends on the specs and n only.
//      Actor and critic choose independently: each has its own rows of partial sums.
//
// Gradient layout (out->actor_grad, out->critic_grad, and a workgroup's row of partial sums): per layer w[out, in] then b[out], hidden
// layers first, the head last; an actor's log_std[6] follows.  A width-16 layer's padded tile rows have no entry.
// Workspace (floats): [actor backward block | critic backward block | actor rows: workgroups_a x part_a | critic rows: workgroups_c x part_c],
// a backward block kPpoMlpBwdFloats (the largest: 52 fragments and 64 zeros), part = grad floats rounded up to 4, plus 4 scalar sums.
#pragma once

#include "rdv_ppo.h"
#include "rdv_ppo_ops.h"

namespace rdv {

constexpr int kPpoMlpBwdFrags = 4 + 3 * 16;                                  // head 2 x 2 x 1, three 64 -> 64 layers 2 x 2 x 4
constexpr int kPpoMlpBwdZero = kPpoMlpBwdFrags * 256, kPpoMlpBwdFloats = kPpoMlpBwdZero + 64;   // 13,376 floats
constexpr int kPpoMlpLdsLimit = 160 * 1024;
static_assert(kPpoMlpBwdFloats % 4 == 0, "the pieces of the workspace are 16-byte aligned");

// The layers of one net as the kernels index them: layer l = 0 .. L (L = n_hidden: the head) is W_l [out_w, in_w].
struct PpoMlpTable {
  int32_t L, waves, grad_floats, part_floats, ls_off, block_floats;
  int32_t in_w[kMlpLayers], out_w[kMlpLayers];     // widths
  int32_t w_off[kMlpLayers], b_off[kMlpLayers];    // where dW_l and db_l start in the flat gradient
  int32_t mt[kMlpLayers], ks[kMlpLayers];          // forward tiles and k-steps (the block's table)
  int32_t bfrag[kMlpLayers + 1];                   // first backward fragment of layer l (1 .. L); [L + 1]: their number
};

// the floats of pack_mlp_weights' block for `spec` (the head is one tile whatever out_dim)
constexpr int ppo_mlp_block_floats(const RdvMlpSpec& spec) {
  int frags = 0, tiles = 0;
  for (int l = 0; l <= spec.n_hidden; ++l) {
    const int mt = l < spec.n_hidden ? mlp_tiles(spec.hidden[l]) : 1, ks = l == 0 ? 2 : mlp_ksteps(spec.hidden[l - 1]);
    frags += 2 * mt * ks; tiles += mt;
  }
  return kMlpHdr + frags * (kPolFragBytes / 4) + tiles * 32;
}
constexpr int ppo_mlp_waves(const RdvMlpSpec& spec) {
  return (ppo_mlp_block_floats(spec) + 8 * kPpoWaveFloats) * 4 <= kPpoMlpLdsLimit ? 8 : 4;
}
inline int ppo_mlp_lds_bytes(const PpoMlpTable& t) { return (t.block_floats + t.waves * kPpoWaveFloats) * 4; }

// (constexpr: rdv_ppo_adam.hip takes the default spec's table at compile time)
// in0: the width of layer 0's input — the 17 observations, or H for the trunk of a recurrent policy (rdv_ppo_lstm.h: H / 16 k-steps)
constexpr void ppo_mlp_table(const RdvMlpSpec& spec, bool actor, PpoMlpTable& t, int in0 = kPolIn) {
  const int L = spec.n_hidden, out_dim = actor ? kPolOut : 1;
  t = PpoMlpTable{};
  t.L = L; t.waves = ppo_mlp_waves(spec); t.block_floats = ppo_mlp_block_floats(spec);
  int at = 0;
  for (int l = 0; l <= L; ++l) {
    t.in_w[l] = l == 0 ? in0 : spec.hidden[l - 1];
    t.out_w[l] = l < L ? spec.hidden[l] : out_dim;
    t.mt[l] = l < L ? mlp_tiles(t.out_w[l]) : 1;
    t.ks[l] = l == 0 ? (in0 == kPolIn ? 2 : in0 / 16) : mlp_ksteps(t.in_w[l]);
    t.w_off[l] = at; at += t.out_w[l] * t.in_w[l];
    t.b_off[l] = at; at += t.out_w[l];
  }
  t.ls_off = actor ? at : -1;
  t.grad_floats = at + (actor ? kPolOut : 0);
  t.part_floats = (t.grad_floats + 3) / 4 * 4 + 4;
  int frag = 0;
  for (int l = 1; l <= L; ++l) {
    t.bfrag[l] = frag;
    frag += 2 * t.mt[l - 1] * (l < L ? t.ks[l + 1] : 1);
  }
  t.bfrag[L + 1] = frag;
}
inline int64_t ppo_mlp_workgroups(const PpoMlpTable& t, int64_t n) { return (n + t.waves * kPolWaveEnvs - 1) / (t.waves * kPolWaveEnvs); }
inline int64_t ppo_mlp_workspace_floats(const PpoMlpTable& a, const PpoMlpTable& c, int64_t n) {
  return 2 * (int64_t)kPpoMlpBwdFloats + ppo_mlp_workgroups(a, n) * a.part_floats + ppo_mlp_workgroups(c, n) * c.part_floats;
}

struct PpoMlpLaunch {
  const float *actor_block, *critic_block;   // the handles' forward parameter blocks (device)
  int actor_act, critic_act;                 // RdvActivation
  PpoMlpTable actor, critic;
  const float *obs, *actions, *old_log_prob, *advantages, *returns;
  const int64_t* indices;                    // nullable
  int64_t n;
  PpoCoefs k;
  float* workspace;
  float *actor_grad, *critic_grad, *scalars, *log_prob, *values;
};

// ---- the set form (rdv_ppo_mlp_set_loss_grad, include/rdv.h "PPO minibatch gradients for policy sets of every MLP architecture"): P
// members of ONE pair of specs in the same four launches, as rdv_ppo.h gives the shipped kernels a set form — the same bodies, the member
// taken from the grid, PpoSetTable (count, off, ws per member) BY VALUE in the kernel arguments, hence the same cap of 64 members.
//   ppo_mlp_set_transpose_kernel   grid (53, 2, P)                                 member z, net y
//   ppo_mlp_net_kernel<.., true>   grid (max_g workgroups_net(counts[g]), P)       workgroup (x, y) is workgroup x of member y's stand-alone
//                                  launch; it returns before its first barrier when it has no rows of that member (workgroup-uniform)
//   ppo_mlp_set_finish_kernel      grid (ceil((Ga + Gc + 1) / 256), P)             member y
// Member y's forward block is set base + y * block_floats (a set allocation holds exactly the bytes of stand-alone handles); its piece of
// the workspace, at table.ws[y], is the stand-alone layout above for n = count[y] (members with count 0 have none); `indices`, log_prob
// and values are advanced by off[y].  The workgroup size stays ppo_mlp_waves of each net's spec, so actor and critic may cut a member's
// rows differently (256 or 128 per workgroup) and their grids differ in x: per member the partition, the wave-order sums and the
// index-order sum of the last kernel are exactly the stand-alone call's, and so is every bit of its outputs.
// Fills `t` for counts[0 .. n_members) (all >= 0, n_members <= kPpoSetMaxMembers) -> the workspace's size in bytes.
inline int64_t ppo_mlp_set_table(const PpoMlpTable& a, const PpoMlpTable& c, int32_t n_members, const int64_t* counts, PpoSetTable* t,
                                 int64_t* max_groups_a = nullptr, int64_t* max_groups_c = nullptr) {
  int64_t off = 0, ws = 0, most_a = 0, most_c = 0;
  for (int g = 0; g < kPpoSetMaxMembers; ++g) {
    const int64_t n = g < n_members ? counts[g] : 0;
    if (t) { t->count[g] = n; t->off[g] = off; t->ws[g] = ws; }
    off += n;
    if (n > 0) ws += ppo_mlp_workspace_floats(a, c, n);
    if (ppo_mlp_workgroups(a, n) > most_a) most_a = ppo_mlp_workgroups(a, n);
    if (ppo_mlp_workgroups(c, n) > most_c) most_c = ppo_mlp_workgroups(c, n);
  }
  if (max_groups_a) *max_groups_a = most_a;
  if (max_groups_c) *max_groups_c = most_c;
  return ws * (int64_t)sizeof(float);
}

struct PpoMlpSetLaunch {
  PpoMlpLaunch a;         // actor_block, critic_block: the sets' allocations; n unused; indices required; actor_grad [P, Ga], critic_grad
                          // [P, Gc], scalars [P, 8]; log_prob, values [sum of counts], nullable
  int32_t n_members;
  int64_t max_groups_a, max_groups_c;
  PpoSetTable table;
};

__attribute__((visibility("hidden"))) hipError_t ppo_mlp_raise_lds_limit();   // the plain and the set instantiations
__attribute__((visibility("hidden"))) void ppo_mlp_launch(const PpoMlpLaunch& a, hipStream_t s);
__attribute__((visibility("hidden"))) void ppo_mlp_set_launch(const PpoMlpSetLaunch& a, hipStream_t s);
// launch 1 alone (the transposed fragments of layers 1 .. L of two blocks -> workspace, 2 kPpoMlpBwdFloats floats): rdv_ppo_lstm.hip's trunks
__attribute__((visibility("hidden"))) void ppo_mlp_launch_transpose(const float* actor_block, const float* critic_block, float* workspace, hipStream_t s);
// ppo_mlp_set_transpose_kernel on its own (rdv_ppo_lstm.hip: the trunks of a recurrent set): member g's blocks, actor_floats / critic_floats
// apart in the sets' allocations -> the backward pair at workspace + table.ws[g]; a member of count 0 is skipped
__attribute__((visibility("hidden"))) void ppo_mlp_launch_set_transpose(const float* actor_set, const float* critic_set, float* workspace, int actor_floats,
                                                                        int critic_floats, int32_t n_members, const PpoSetTable& table, hipStream_t s);


// ---------------------------------------------------------------------------------------------------------------- device
// The steps of a net kernel that do not depend on what layer 0 reads: the kept forward layers and one backward step.  rdv_ppo_mlp.hip
// (layer 0 over the observation rows) and rdv_ppo_lstm.hip (the trunk of a recurrent policy: layer 0 over h_t) both take them.
// mlp_hidden with the activations of its MT tiles kept
template <int ACT, int MT, int KS>
__device__ __forceinline__ void mlp_hidden_keep(const float* wf, const float* zerop, int frag0, const float* biasp, float k, int lane, f16x8 (&x)[4][2],
                                                float (&hs)[2][16]) {
  f16x8 xin[KS][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) { xin[ks][0] = x[ks][0]; xin[ks][1] = x[ks][1]; }
  f32x16 d[MT];
  layer<MT, KS>(wf, frag0, zerop, xin, lane, d);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mlp_add_bias(d[mt], biasp + (mt * 2 + (lane >> 5)) * 16);
    ppo_activate_keep<ACT>(d[mt], k, x[2 * mt], x[2 * mt + 1], hs[mt]);
  }
}
// hidden layers `from` .. `upto` - 1 of the block at `w` on x (the B fragments of layer `from`'s input): x <- the B fragments of h_upto,
// hs <- h_upto (times 2^10) in accumulator order
template <int ACT>
__device__ __forceinline__ void mlp_layers_keep(const float* w, const int32_t* __restrict__ H, int lane, int from, int upto, f16x8 (&x)[4][2],
                                                float (&hs)[2][16]) {
  const float* wf = w + kMlpHdr;
  const float* zerop = w + kMlpZero;
#pragma nounroll
  for (int l = from; l < upto; ++l) {
    const int32_t* rec = H + kMlpRec + kMlpRecStride * l;
    const int frag0 = rec[0];
    const float* biasp = w + rec[1];
    const float k = mlp_act_const<ACT>(__int_as_float(rec[4]));
    switch (rec[2] * 8 + rec[3]) {
      case 8 + 1: mlp_hidden_keep<ACT, 1, 1>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
      case 8 + 2: mlp_hidden_keep<ACT, 1, 2>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
      case 8 + 4: mlp_hidden_keep<ACT, 1, 4>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
      case 16 + 1: mlp_hidden_keep<ACT, 2, 1>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
      case 16 + 2: mlp_hidden_keep<ACT, 2, 2>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
      default: mlp_hidden_keep<ACT, 2, 4>(wf, zerop, frag0, biasp, k, lane, x, hs); break;
    }
  }
}
// mlp_means up to hidden layer `upto` (1 .. L): x <- the B fragments of h_upto, hs <- h_upto (times 2^10) in accumulator order
template <int ACT>
__device__ __forceinline__ void mlp_forward_keep(const float* w, const int32_t* __restrict__ H, const float* rows, int lane, int upto, f16x8 (&x)[4][2],
                                                 float (&hs)[2][16]) {
  {
    f16x8 x0[2][2];
    actor_inputs(rows, lane, x0);
#pragma unroll
    for (int q = 0; q < 2; ++q) { x[0][q] = x0[0][q]; x[1][q] = x0[1][q]; x[2][q] = (f16x8)(0); x[3][q] = (f16x8)(0); }
  }
  mlp_layers_keep<ACT>(w, H, lane, 0, upto, x, hs);
}

// The derivative of the activation from the forward's own activation (hs = h 2^10): tanh 1 - h^2; sigmoid h (1 - h); ReLU 1 where
// 0 < h < 63 — PyTorch's 0 at the kink, and 0 where the kernel's [0, 63] cap acted.  A NaN activation gives 0 for the ReLU; the error it
// multiplies is a NaN already (the NaN reached the head), and NaN x 0 stays NaN.
template <int ACT>
__device__ __forceinline__ float mlp_act_derivative(float hs) {
  constexpr float one = (float)(1 << kPolXShift), inv = 1.0f / one;
  if (ACT == RDV_ACT_RELU) return (hs > 0.0f && hs < 63.0f * one) ? 1.0f : 0.0f;
  const float hv = hs * inv;
  if (ACT == RDV_ACT_TANH) return 1.0f - hv * hv;
  return hv * (1.0f - hv);
}

// One backward step, layer l >= 1 (l == L: the head), MTh tiles of h_l, KSd k-steps and MTd tiles of delta_l (KSd = 4 <=> MTd = 2):
//   dl (delta_l times n, in) is scaled by the wave's S;  pre = W_l^T dl (the forward's `layer` on the transposed fragments);
//   delta_{l-1} = pre o act'(h_l) 2^-s_l / S;  dW_l, db_l (the head of an actor: d log_std from tile rows 8..13) -> the workgroup's row;
//   dl <- delta_{l-1}.
template <int ACT, bool ACTOR, int MTh, int KSd>
__device__ __forceinline__ void backward_step(const PpoMlpTable& T, int l, const float* bwd, float inv_acc, float (&dl)[2][16], const float (&hs)[2][16],
                                              float* wave_tiles, const float* tiles0, int nw, int lane, float* part) {
  constexpr int MTd = KSd == 4 ? 2 : 1;
  constexpr float xs = (float)(1 << kPolXShift), inv_xs = 1.0f / xs;
  const bool head = l == T.L;
  float S, invS;
  wave_scale(MTd == 2 ? fmaxf(tile_max(dl[0]), tile_max(dl[1])) : tile_max(dl[0]), S, invS);
#pragma unroll
  for (int mt = 0; mt < MTd; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dl[mt][e] *= S;
  float nd[MTh][16];
  {
    f16x8 b[KSd][2];
    if constexpr (KSd == 1) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = (head && j >= 4) ? 0.0f : dl[0][j];   // the head's d log_std terms stay out of the product
      split2(x, b[0]);
    } else {
#pragma unroll
      for (int s = 0; s < KSd; ++s) error_frags(dl[s >> 1], s & 1, b[s]);
    }
    f32x16 pre[MTh];
    layer<MTh, KSd>(bwd, T.bfrag[l], bwd + kPpoMlpBwdZero, b, lane, pre);
    const float un = inv_acc * xs * invS;                                      // 2^-s_l / S
#pragma unroll
    for (int mt = 0; mt < MTh; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) nd[mt][e] = pre[mt][e] * mlp_act_derivative<ACT>(hs[mt][e]) * un;
  }
  {
    _Float16* tb = reinterpret_cast<_Float16*>(wave_tiles);
#pragma unroll
    for (int mt = 0; mt < MTh; ++mt) stage_tile(tb + mt * (2 * kPpoTile), hs[mt], lane);
    const int w_off = T.w_off[l], b_off = T.b_off[l], in_w = T.in_w[l], out_w = T.out_w[l], ls_off = T.ls_off;
    weight_grads<MTd, MTh, 0>(dl, wave_tiles, tiles0, nw, invS * inv_xs, lane, [&](int row, int col, float v) {
      if (col >= 0) { if (row < out_w && col < in_w) part[w_off + row * in_w + col] = v; }
      else if (col == -1) {
        if (row < out_w) part[b_off + row] = v;
        if (ACTOR && head && row >= 8 && row < 8 + kPolOut) part[ls_off + (row - 8)] = v;
      }
    });
  }
#pragma unroll
  for (int mt = 0; mt < MTh; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dl[mt][e] = nd[mt][e];
}

}  // namespace rdv

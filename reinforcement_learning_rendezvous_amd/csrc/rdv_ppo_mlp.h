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
constexpr void ppo_mlp_table(const RdvMlpSpec& spec, bool actor, PpoMlpTable& t) {
  const int L = spec.n_hidden, out_dim = actor ? kPolOut : 1;
  t = PpoMlpTable{};
  t.L = L; t.waves = ppo_mlp_waves(spec); t.block_floats = ppo_mlp_block_floats(spec);
  int at = 0;
  for (int l = 0; l <= L; ++l) {
    t.in_w[l] = l == 0 ? kPolIn : spec.hidden[l - 1];
    t.out_w[l] = l < L ? spec.hidden[l] : out_dim;
    t.mt[l] = l < L ? mlp_tiles(t.out_w[l]) : 1;
    t.ks[l] = l == 0 ? 2 : mlp_ksteps(t.in_w[l]);
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

}  // namespace rdv

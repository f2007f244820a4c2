// rdv_ppo_lstm.h — the PPO loss of one minibatch of whole env columns of a recurrent rollout and its gradients for every parameter of a
// stand-alone recurrent actor and critic (rdv_policy_lstm.h: an LSTM of H = 32 / 64 / 128 / 256 in front of an RdvMlpSpec trunk, each net
// with an LSTM of its own), back-propagated through time (rdv_lstm_ppo_loss_grad, include/rdv.h "Recurrent PPO minibatch gradients").
// The kernels are in rdv_ppo_lstm.hip, a translation unit of its own; this header holds the sizes, the workspace layout and the launch
// that the host unit needs, and the description.  The products follow rdv_policy_lstm.h and rdv_ppo_ops.h: two fp16 terms per operand
// (split2), three MFMAs per k-step (mfma3), error operands scaled by a power of two per wave (wave_scale) and staged through the LDS
// operand tiles (stage_tile, load_frags), transposed fragments derived on the device from the handle's forward block, sums in a fixed
// order (waves in wave order, workgroups in index order through the workspace) and no floating-point atomic.
//
// A minibatch is B env columns of a [T, N] rollout, all T steps each: n = T B rows, row m = t B + b.  Per net (actor, critic) the launches:
//   0. (once for both nets) lstm_ppo_gather_kernel: the observations of the columns -> obs_g [T][B 17, padded to 4 floats] (the cell
//      kernel reads contiguous 16-byte aligned rows), s_t -> start_g [T][B] (row 0: zeros — state0 is given as step 0 sees it; row t:
//      done[t-1]), state0 of the columns -> h0_g, c0_g [B, H];  ppo_mlp_transpose_kernel (rdv_ppo_mlp.hip, as it is): the transposed
//      fragments of the trunks' layers 1 .. L;  lstm_ppo_transpose_kernel: the transposed fragments of W_hh (K = the 4 H gate rows in
//      natural order, H / 32 output tiles) and of the trunk's layer 0 (K = hidden[0] in accumulator order, H / 32 output tiles).
//   1. Forward replay: T launches of lstm_cell_keep_kernel — the body of lstm_cell_kernel (rdv_policy_lstm.h) restated statement for
//      statement with the gate activations kept (not a shared function: that kernel's instruction stream is pinned to a recorded digest,
//      and a common body changes its register allocation; tests/test_gpu_ppo_lstm_grad.py holds the replayed values to the rollout's bits
//      for every H) — on the gathered rows: h_t, c_t -> hs, cs [T B, H], the gate activations -> gates [T B, 4 H].  The handle's own state and pending flags
//      are neither read nor written.
//   2. lstm_ppo_trunk_kernel<ACT, ACTOR>: all T B rows, a wave 32 rows, eight waves a workgroup.  The loop of ppo_mlp_net_kernel over the
//      layers from the head down with its functions (mlp_layers_keep, ppo_loss_terms, backward_step), layer 0 read from h_t over H / 16
//      k-steps with the operations of lstm_trunk_first; behind it layer 0's own step: d loss / d h_t = W_0^T delta_0 -> dh [T B, H],
//      dW_0 = delta_0 h_t^T two column tiles at a time through weight_grads.  The workgroup's sums go to its row of the workspace.
//   3. Backward through time: T launches of lstm_ppo_bptt_kernel<H>, t = T-1 .. 0, a wave 32 columns.  Per block of 32 units:
//      rec = W_hh^T da_{t+1} (4 H / 16 k-steps on the transposed fragments, da_{t+1} scaled by the wave's power of two that step t + 1
//      left in `dscale`, zero where done[t] cuts the flow), dh_t = dh_t(trunk) + rec; then element-wise, from the forward's own
//      activations: do = dh tanh(c_t), dc = dh o (1 - tanh^2 c_t) + (1 - done[t]) f_{t+1} dc_{t+1}; da_i = dc g i (1 - i),
//      da_f = dc c_{t-1} f (1 - f), da_g = dc i (1 - g^2), da_o = do o (1 - o); da_t overwrites the gates of step t, f_t dc_t -> dcc.
//   4. lstm_ppo_wgrad_kernel: [dW_ih | db | dW_hh] = sum over the T B rows of da_t [x_t | 1 | (1 - s_t) h_{t-1}]^T, a contraction with
//      K = T B.  Workgroup (mt, nt, split) owns the 32 x 32 output tile (rows 32 mt of the 4 H gate rows; nt = 0: the 17 inputs clamped to
//      +-63 as the forward reads them, and a column of ones; nt >= 1: units 32 (nt - 1) of h_{t-1}) for the 32-row chunks
//      split 8 + wave, + 8 splits, ...: per chunk the da tile scaled by its wave_scale, both tiles staged and read back as fragments, six
//      MFMAs, the product unscaled and added to the wave's fp32 sum; the eight waves' sums added in wave order -> the split's row of
//      partial sums.  b_ih and b_hh get the same gradient.
//   5. (once) lstm_ppo_finish_kernel: per gradient element the trunk rows in workgroup order or the cell rows in split order, divided by
//      n; - ent_coef on d log_std; the scalars in double (ppo_finish_scalars).
// Launches: 4 T + 8 (3 + 2 (T + 1 + T + 1) + 1), fixed by the specs, T and B.  The set form below (rdv_lstm_ppo_set_loss_grad): the same
// 4 T + 8 whatever the number of members.
//
// Decisions:
//   Kept or recomputed: the gate activations are KEPT.  Per row and net the workspace holds h, c (2 H floats), the gates (4 H, later da
//      in their place) and dh (H): 28 H bytes — 7 KiB at H = 256, 0.9 KiB at H = 32 — so T = 128, B = 2048, H = 256 takes 1.8 GiB per net.
//      Keeping h and c alone would take 12 H bytes per row and repeat the cell's 12 (2 + H / 16) MFMAs per block of 32 units in every
//      backward step, next to the 12 H / 16 MFMAs per block of the W_hh^T product: twice the matrix work of a step and a second pass over
//      the gate weights, on the path that is T launches long.  The backward step is the latency-bound part (one workgroup per 256
//      columns), and memory is not what a minibatch of columns runs out of first, so the step stays short.
//   Weights from device memory, as the forward: the W_hh^T fragments are the size of W_hh's (1 MiB at H = 256) and L2-resident; a wave
//      reads each as full 1 KiB lines.  No kernel here stages weights in LDS.
//   LDS and occupancy: the cell kernel as in the rollout (17 KiB static).  The trunk kernel: eight waves x (three operand tiles + 4 sums)
//      = 98,432 B dynamic: ONE workgroup of eight waves per CU (160 KiB), two waves per SIMD, as ppo_mlp_net_kernel; its registers are that
//      kernel's (x, one layer's h, one error tile set) under __launch_bounds__(512), the 256 unified registers two waves per SIMD leave a
//      wave: 244 (critic) to 256 (actor), no scratch (the row's addresses are formed where they are used).  The BPTT kernel has no LDS and one 16-register
//      accumulator at a time, 102 - 122 VGPRs: four waves per SIMD, but a minibatch of B columns fills only B / 256 workgroups: it is
//      latency-bound by the recurrence itself.  The weight-gradient kernel (97 VGPRs): eight waves x two tiles = 64 KiB static
//      (the product overwrites the wave's A tile), two workgroups per CU; 4 H / 32 x (1 + H / 32) x splits workgroups — 288 x splits at
//      H = 256, 8 x splits at H = 32, splits = ceil(chunks / 64) capped at 16.
//
// Gradient layout (out->actor_grad, out->critic_grad): w_ih[4H,17] w_hh[4H,H] b_ih[4H] b_hh[4H], then the trunk as rdv_ppo_mlp.h lays a
// net out with layer 0 = [hidden[0], H] (per layer w[out, in] then b[out], the head last), log_std[6] last for an actor.
// Accuracy: tests/test_gpu_ppo_lstm_grad.py holds every tensor to err = max|G - G64| / max|G64| <= C max(e32, 2^-23), C = 32 (tensors) and
// 128 (scalars), the constants of rdv_ppo_mlp for the same operand precision; profiles/lstm_ppo_grad_accuracy.csv has the measured ratios.
#pragma once

#include "rdv_policy_lstm.h"
#include "rdv_ppo_mlp.h"

namespace rdv {

constexpr int kLstmPpoMaxSplits = 16;

// the sizes of one net
struct LstmPpoNet {
  int32_t H, cell_floats, cell_part, w0t_floats, whht_floats, grad_floats;
  PpoMlpTable T;   // the trunk, layer 0 = [hidden[0], H]; its offsets are relative to the trunk's first gradient float (cell_floats)
};
inline void lstm_ppo_net(int H, const RdvMlpSpec& trunk, bool actor, LstmPpoNet& n) {
  n.H = H;
  ppo_mlp_table(trunk, actor, n.T, H);
  n.T.waves = 8; n.T.block_floats = 0;                       // (no block in LDS here: eight waves whatever the trunk)
  n.cell_floats = 4 * H * kPolIn + 4 * H * H + 8 * H;
  n.cell_part = 4 * H * kPolIn + 4 * H * H + 4 * H;          // one bias gradient: b_ih and b_hh share it
  n.w0t_floats = 2 * (H / 32) * mlp_ksteps(trunk.hidden[0]) * (kPolFragBytes / 4);
  n.whht_floats = 2 * (H / 32) * (4 * H / 16) * (kPolFragBytes / 4);
  n.grad_floats = n.cell_floats + n.T.grad_floats;
}
__host__ __device__ inline int64_t lstm_ppo_up4(int64_t x) { return (x + 3) / 4 * 4; }
__host__ __device__ inline int lstm_ppo_splits(int64_t n) {
  const int64_t chunks = (n + 31) / 32, s = (chunks + 63) / 64;
  return (int)(s < 1 ? 1 : (s > kLstmPpoMaxSplits ? kLstmPpoMaxSplits : s));
}
// the trunk kernel's workgroups for n rows: eight waves of 32 rows (ppo_mlp_workgroups of a table with waves = 8)
__host__ __device__ inline int64_t lstm_ppo_trunk_groups(int64_t n) { return (n + 8 * kPolWaveEnvs - 1) / (8 * kPolWaveEnvs); }

// The workspace (floats; every piece starts at a multiple of 4): [actor trunk bwd | critic trunk bwd] (ppo_mlp_transpose_kernel's pair),
// obs_g, start_g, then per net: w0t, whht, h0_g, c0_g, hs, cs, gates, dh, dcc, dscale, trunk rows, cell rows.
// LstmPpoDims: what the layout needs of the two nets (index 0 actor, 1 critic), small enough to travel by value: the set form evaluates
// the layout of each member's piece on the device from (T, B_g).  One definition, host and device.
struct LstmPpoDims { int32_t H[2], w0t[2], whht[2], tpart[2], cpart[2]; };   // units; floats of W_0^T, of W_hh^T, of a trunk row, of a cell row
struct LstmPpoNetWs { int64_t w0t, whht, h0, c0, hs, cs, gates, dh, dcc, dscale, tparts, cparts; };
struct LstmPpoHeadWs { int64_t obs, start, obs_stride, end; };
struct LstmPpoWs { int64_t obs, start, total; int64_t obs_stride; LstmPpoNetWs net[2]; };
inline LstmPpoDims lstm_ppo_dims(const LstmPpoNet& a, const LstmPpoNet& c) {
  return {{a.H, c.H}, {a.w0t_floats, c.w0t_floats}, {a.whht_floats, c.whht_floats}, {a.T.part_floats, c.T.part_floats},
          {(int32_t)lstm_ppo_up4(a.cell_part), (int32_t)lstm_ppo_up4(c.cell_part)}};
}
__host__ __device__ inline LstmPpoHeadWs lstm_ppo_head_layout(int64_t T, int64_t B) {
  LstmPpoHeadWs h;
  int64_t at = 2 * (int64_t)kPpoMlpBwdFloats;
  h.obs_stride = lstm_ppo_up4(B * kPolIn);
  h.obs = at; at += T * h.obs_stride;
  h.start = at; at += lstm_ppo_up4((T * B + 3) / 4);
  h.end = at;
  return h;
}
// net k's pieces from float `at` on -> where the next net's start
__host__ __device__ inline int64_t lstm_ppo_net_layout(const LstmPpoDims& d, int k, int64_t T, int64_t B, int64_t at, LstmPpoNetWs& o) {
  const int64_t n = T * B, H = d.H[k];
  o.w0t = at; at += d.w0t[k];
  o.whht = at; at += d.whht[k];
  o.h0 = at; at += B * H;
  o.c0 = at; at += B * H;
  o.hs = at; at += n * H;
  o.cs = at; at += n * H;
  o.gates = at; at += n * 4 * H;
  o.dh = at; at += n * H;
  o.dcc = at; at += B * H;
  o.dscale = at; at += lstm_ppo_up4(T * ((B + 31) / 32));
  o.tparts = at; at += lstm_ppo_trunk_groups(n) * d.tpart[k];
  o.cparts = at; at += (int64_t)lstm_ppo_splits(n) * d.cpart[k];
  return at;
}
inline void lstm_ppo_workspace(const LstmPpoNet& a, const LstmPpoNet& c, int64_t T, int64_t B, LstmPpoWs& w) {
  const LstmPpoDims d = lstm_ppo_dims(a, c);
  const LstmPpoHeadWs h = lstm_ppo_head_layout(T, B);
  w.obs = h.obs; w.start = h.start; w.obs_stride = h.obs_stride;
  w.total = lstm_ppo_net_layout(d, 1, T, B, lstm_ppo_net_layout(d, 0, T, B, h.end, w.net[0]), w.net[1]);
}

struct LstmPpoLaunch {
  const float *actor_block, *critic_block;   // the handles' forward blocks (device): [trunk block | cell block]
  int actor_act, critic_act;
  LstmPpoNet actor, critic;
  const float *obs, *actions, *old_log_prob, *advantages, *returns;   // [T, N, ..]
  const uint8_t* done;                                                // [T, N]
  const float *actor_h0, *actor_c0, *critic_h0, *critic_c0;           // [N, H]
  const int64_t* envs;                                                // [B], nullable
  int64_t n_envs, n_steps, n_seq;
  PpoCoefs k;
  float* workspace;
  float *actor_grad, *critic_grad, *scalars, *log_prob, *values;
};

__attribute__((visibility("hidden"))) hipError_t lstm_ppo_raise_lds_limit();
__attribute__((visibility("hidden"))) void lstm_ppo_launch(const LstmPpoLaunch& a, hipStream_t s);

// ---- the set form (rdv_lstm_ppo_set_loss_grad, include/rdv.h "Recurrent PPO minibatch gradients for recurrent sets"): P members'
// minibatches of whole columns in the same 4 T + 8 launches.  Every kernel above has a SET form (the cell step: lstm_cell_keep_set_kernel on
// the same lstm_cell_rows; the trunks' layers 1 .. L: ppo_mlp_set_transpose_kernel as it is): the member is taken from the grid — blockIdx.y,
// blockIdx.z where y is taken, blockIdx.z / the widest member's splits in the weight-gradient kernel — and the body runs on that member's
// arguments, so workgroup (x, member) IS workgroup x of the member's stand-alone launch: its partition into waves and workgroups, its
// wave_scale values, its lstm_ppo_splits(T B_g) and its wave-order and index-order sums.  Hence member g's outputs are, bit for bit, what
// rdv_lstm_ppo_loss_grad writes for stand-alone handles with its weights, envs + off_g and n_seq = B_g.  A workgroup beyond the member's
// own count (a narrower member, a split index >= its splits, a member without columns) returns before the first barrier; the condition
// is workgroup-uniform.  Member g's forward block is the set's allocation + g block_floats; its piece of the workspace is the stand-alone
// layout for (T, B_g) at table.ws[g], member after member (members of count 0 left out), evaluated on the device (lstm_ppo_head_layout,
// lstm_ppo_net_layout: scalar arithmetic on kernel arguments).  count, off (in columns) and ws travel BY VALUE (PpoSetTable, rdv_ppo.h):
// no device table, no copy, hence the same cap of 64 members.  Outputs: row g of actor_grad [P, Ga], critic_grad [P, Gc], scalars [P, 8];
// log_prob and values: member g's [T, B_g] block at float T off_g.  Nothing of a member without columns is written.
struct LstmPpoSetCommon {
  const float* block[2];     // the sets' allocations (actor, critic)
  int32_t block_floats[2];   // a member's forward block
  float* ws;                 // the workspace
  int64_t T;
  LstmPpoDims d;
  PpoSetTable table;
};
struct LstmPpoSetLaunch {
  LstmPpoLaunch a;           // actor_block, critic_block: the sets' allocations; envs required, all members'; n_seq unused; the outputs' row 0
  int32_t n_members, actor_block_floats, critic_block_floats;
  int64_t max_count;         // the widest member's columns
  PpoSetTable table;
};
// fills `t` for counts[0 .. n_members) (all >= 0, n_members <= kPpoSetMaxMembers) -> the workspace's size in bytes: the sum of the members'
inline int64_t lstm_ppo_set_table(const LstmPpoNet& a, const LstmPpoNet& c, int64_t T, int32_t n_members, const int64_t* counts, PpoSetTable* t,
                                  int64_t* max_count = nullptr) {
  int64_t off = 0, ws = 0, most = 0;
  for (int g = 0; g < kPpoSetMaxMembers; ++g) {
    const int64_t B = g < n_members ? counts[g] : 0;
    if (t) { t->count[g] = B; t->off[g] = off; t->ws[g] = ws; }
    off += B;
    if (B > 0) {
      LstmPpoWs w;
      lstm_ppo_workspace(a, c, T, B, w);
      ws += w.total;
    }
    if (B > most) most = B;
  }
  if (max_count) *max_count = most;
  return ws * (int64_t)sizeof(float);
}
__attribute__((visibility("hidden"))) void lstm_ppo_set_launch(const LstmPpoSetLaunch& L, hipStream_t s);

}  // namespace rdv

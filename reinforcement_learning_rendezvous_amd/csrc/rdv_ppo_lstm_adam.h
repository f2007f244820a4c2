// rdv_ppo_lstm_adam.h — the optimiser half of a recurrent sweep's update step (rdv_lstm_ppo_set_adam_step, include/rdv.h "Gradient clip, Adam
// and weight repack for recurrent policy sets"): what rdv_ppo_adam.h does for MLP sets, for all P members of a recurrent actor set and a
// recurrent critic set at once — clip_grad_norm_ over the member's parameters, Adam, and the repack of its two forward blocks
// [trunk block | cell block] (rdv_policy_lstm.h), a device restatement of pack_lstm_weights.  The kernels are in rdv_ppo_lstm_adam.hip, a
// translation unit of its own; this header holds the sizes, the workspace layout and the launch that the host unit needs.
//
// ppo_adam_update_kernel keeps a net's parameters in LDS (at most 14,028 floats); a recurrent net has 13 k floats at H = 32 and 302 k at
// H = 256 with a [64, 64] trunk, so here a member is spread over many workgroups and the fp32 master rows in device memory (L2-resident
// between the launches) are what the repack gathers from.  Rows are Ga / Gc floats long (rdv_lstm_ppo_grad_floats), back to back, hence
// 4-byte aligned only: every access to them is one float.  FOUR launches per call, all on the caller's stream, whatever P and the specs:
//   1. lstm_adam_sumsq_kernel  grid (sum_chunks, P), 256 threads.  Chunk c of member g is the entries [4096 c, 4096 (c + 1)) of the
//      concatenation [actor row | critic row] of its gradients; thread t adds the squares of the chunk's entries t, t + 256, .. in index
//      order in double, the 256 sums are added by a fixed tree (ppo_adam_norm_kernel's), the chunk's sum goes to the workspace.
//   2. lstm_adam_coef_kernel   grid (P), one wave.  The chunk sums added in index order in double, then adam_member_coef — the function
//      ppo_adam_norm_kernel ends in: total_norm, clip_coef, the two step coefficients, coef[g], step[g] <- step[g] + 1, or the skip.
//   3. lstm_adam_step_kernel   grid (chunks, 2, P), 256 threads.  Workgroup (c, net, g): adam_element (rdv_ppo_adam.h, the four float32
//      lines) on the entries [4096 c, 4096 (c + 1)) of the net's row, 16 per thread, coalesced; m, v, p back to the caller's rows; the
//      chunk's max |p_new| per PACKER LAYER — 0: the cell's [W_ih | W_hh], 1 + l: the trunk's layer l — to the workspace (a chunk may
//      straddle layers; a layer it does not touch gets 0; a maximum has no order).
//   4. lstm_adam_pack_kernel   grid (item chunks, 2, P), 256 threads.  Every workgroup reduces the net's partial maxima to the L + 2 shifts
//      (adam_shift; the cell has ONE shift: the rule is monotone, so the shift of max(max|W_ih|, max|W_hh|) is min(s_ih, s_hh)), then
//      thread q of the net's items builds one of: the 16 bytes that lane (q & 63) of fragment (q >> 6) reads — the trunk's fragments layer
//      by layer ([term][mt][ks], layer 0 natural k over H / 16 k-steps, later layers accumulator order), then the cell's
//      ([term][tile = q H / 32 + j][ks], k-steps 0, 1 the 17 inputs zero-padded, then h) — eight weights gathered from the member's master
//      row, split by adam_split_term; one bias float (the trunk's [mt][h][16] per layer, then b_ih, then b_hh, [tile][h][16], times the
//      accumulator's scale); one inverse scale (each trunk layer's record, the cell block's float 0); an actor's exp(log_std) (the
//      double-precision exp rounded to float) and log_std.  Only live floats are written: header words, the H word of the cell header,
//      the kMlpZero floats and the record integers are the host packer's.
// No floating-point atomic, nothing read from the forward blocks, no LDS beyond the reductions (2 KiB in launch 1, < 200 B in 3 and 4), so
// occupancy is bound by registers alone; no scratch.  At H = 256 with [64, 64] trunks launch 3 has 74 x 2 x P workgroups and launch 4
// about 310 x 2 x P; at H = 32 they have 4 x 2 x P and about 28 x 2 x P.
//
// The workspace (the caller's, 16-byte aligned): member g's slice at g * member_bytes — sum_chunks doubles (the chunk sums of launch 1),
// padded to 16 bytes, then 2 x (kMlpLayers + 1) x chunks floats (the partial maxima, [net][packer layer][chunk], chunks = the longer net's), padded
// to 16 bytes.  An inactive member's slice is not touched.
#pragma once

#include "rdv_policy_lstm.h"
#include "rdv_ppo_adam.h"
#include "rdv_ppo_lstm.h"

namespace rdv {

constexpr int kLstmAdamChunk = 4096;                 // entries per workgroup of launches 1 and 3: 16 per thread
constexpr int kLstmAdamPerThread = kLstmAdamChunk / kPpoAdamThreads;
constexpr int kLstmAdamPackLayers = kMlpLayers + 1;  // the cell, then the trunk's layers
constexpr int kLstmAdamLaunches = 4;

// one net as launches 3 and 4 index it
struct LstmAdamNet {
  int32_t H, cell_w, cell_floats, grad_floats;       // cell_w: the floats of [W_ih | W_hh]; cell_floats: those plus b_ih, b_hh = where the trunk starts
  int32_t block_floats, cell_at;                     // a member's forward block; where its cell block starts (the trunk block's floats)
  int32_t frags_trunk, frags_all, tiles_trunk, cell_tiles, cell_ks;
  int32_t items, chunks;                             // launch 4's thread-items; launch 3's chunks
  int32_t frag0[kMlpLayers + 1], tile0[kMlpLayers + 1];   // the first fragment / bias tile of trunk layer l; [L + 1]: their number
  PpoMlpTable T;                                     // the trunk, layer 0 = [hidden[0], H]; offsets relative to cell_floats
};
inline void lstm_adam_net(int H, const RdvMlpSpec& trunk, bool actor, LstmAdamNet& n) {
  LstmPpoNet g;
  lstm_ppo_net(H, trunk, actor, g);
  n = LstmAdamNet{};
  n.H = H; n.T = g.T;
  n.cell_w = 4 * H * kPolIn + 4 * H * H; n.cell_floats = g.cell_floats; n.grad_floats = g.grad_floats;
  int frags = 0, tiles = 0;
  for (int l = 0; l <= n.T.L; ++l) {
    n.frag0[l] = frags; n.tile0[l] = tiles;
    frags += 2 * n.T.mt[l] * n.T.ks[l]; tiles += n.T.mt[l];
  }
  n.frag0[n.T.L + 1] = frags; n.tile0[n.T.L + 1] = tiles;
  n.frags_trunk = frags; n.tiles_trunk = tiles;
  n.cell_tiles = lstm_cell_tiles(H); n.cell_ks = lstm_cell_ksteps(H);
  n.frags_all = frags + 2 * n.cell_tiles * n.cell_ks;
  n.cell_at = kMlpHdr + frags * (kPolFragBytes / 4) + tiles * 32;
  n.block_floats = n.cell_at + (int32_t)lstm_cell_floats(H);
  n.items = n.frags_all * 64 + tiles * 32 + 2 * n.cell_tiles * 32 + (n.T.L + 2) + (actor ? kPolOut : 0);
  n.chunks = (n.grad_floats + kLstmAdamChunk - 1) / kLstmAdamChunk;
}

struct LstmAdamLaunch {
  PpoAdamLaunch a;                                   // the blocks, the caller's arrays, the mask and the scalars, as rdv_ppo_adam.h's launches take them
  LstmAdamNet net[2];                                // actor, critic
  char* ws;
  int64_t member_bytes;                              // a member's slice of the workspace
  int32_t sum_chunks, chunks, maxima_at;             // launch 1's chunks; the longer net's chunks; the byte offset of the partial maxima in a slice
};
static_assert(sizeof(LstmAdamLaunch) <= 4096, "the arguments fit the 4 KiB kernel-argument segment");

// fills the workspace fields of L from its two nets -> the bytes P members need
inline int64_t lstm_adam_workspace(LstmAdamLaunch& L, int32_t n_members) {
  const int64_t total = (int64_t)L.net[0].grad_floats + L.net[1].grad_floats;
  L.sum_chunks = (int32_t)((total + kLstmAdamChunk - 1) / kLstmAdamChunk);
  L.chunks = L.net[0].chunks > L.net[1].chunks ? L.net[0].chunks : L.net[1].chunks;
  L.maxima_at = (L.sum_chunks * 8 + 15) / 16 * 16;
  L.member_bytes = L.maxima_at + ((int64_t)2 * kLstmAdamPackLayers * L.chunks * 4 + 15) / 16 * 16;
  return L.member_bytes * n_members;
}

__attribute__((visibility("hidden"))) void lstm_adam_launch(const LstmAdamLaunch& L, hipStream_t s);

}  // namespace rdv

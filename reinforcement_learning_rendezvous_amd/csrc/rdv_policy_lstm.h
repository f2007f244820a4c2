// rdv_policy_lstm.h — the reference's recurrent policy (main_rnn.py: sb3-contrib RecurrentPPO("MlpLstmPolicy"), one LSTM layer of
// H = 32 / 64 / 128 / 256 in front of the mlp_extractor trunk, separate actor and critic LSTMs; RdvLstmSpec in include/rdv.h) on the
// scheme of rdv_policy.h and rdv_policy_mlp.h, with their functions: power-of-two scaling, two fp16 terms per operand (split2), three
// v_mfma_f32_32x32x16_f16 per k-step (mfma3), transposed products with a 32-env tile per wave as the B operand, tanh2_f32 and the
// sigmoid of mlp_act2, mlp_hidden / mlp_head for the trunk behind its first layer, actor_outputs for noise, clip and stores.
//
// Two launches per call, the state going through the handle's buffers:
//   lstm_cell_kernel<H>     h, c <- (1 - s) h, (1 - s) c;  a = W_ih x + b_ih + W_hh h + b_hh;  c' = sig(a_f) c + sig(a_i) tanh(a_g);
//                           h' = sig(a_o) tanh(c').  Per block of 32 hidden units the four gate tiles (rows q H + 32 j .. + 31, q = i, f,
//                           g, o) accumulate side by side — 64 accumulator registers — over the 2 k-steps of the 17 inputs and the
//                           H / 16 k-steps of h; the cell update is element-wise on those registers; c is read and written once, in
//                           accumulator order.  h' goes to a buffer of its own (h_next): the other blocks of the same wave still read h.
//   lstm_trunk_kernel<ACT, CRITIC>   latent = h_next -> the trunk (first layer [hidden[0], H] over H / 16 k-steps, then mlp_hidden /
//                           mlp_head) -> actions / value; when the call commits, the rows of h_next it has just read become h.
// A call that does not commit (rdv_lstm_value with commit = 0) has the cell kernel write c' into a scratch buffer and the trunk kernel
// leave h alone: h and c are then never written.  The state is fp32, row-major [rows, H], owned by the handle.
// Recurrent sets (several networks, each owning a range of rows): the same two kernels with one more argument, see LstmSetBlocks below.
//
// The B operand of the h k-steps is read from the state as it lies: lane (r, hh) of k-step ks takes the 8 floats h[r][16 ks + 8 hh ..]
// (two 16-byte loads), times 2^10, clamped to +-63 as an input is (|h| < 1 unless rdv_lstm_set_state put something else there; a NaN
// stays NaN and stays in its env's column of every product).  The weights are packed in that natural k order, as a first MLP layer is.
// A block re-reads and re-splits h (H / 32 times per call): ~35 vector instructions per k-step beside its 12 MFMAs of 8 passes.
//
// Weights.  Gate fragments with two fp16 terms are 2 x 4 H / 32 x (2 + H / 16) KiB: 24 KiB at H = 32, 96 KiB at 64, 320 KiB at 128,
// 1.1 MiB at 256 — only the first two fit a CU's LDS, so ONE path serves every H: each wave reads its fragments straight from device
// memory (the block is L2-resident; a fragment is 1 KiB, lane l its 16 bytes at 16 l: every read is a full coalesced line).  The trunk's
// block is read the same way (its first layer alone is up to 64 KiB at H = 256).  W_ih and W_hh share one power-of-two scale (they
// add up in one accumulator); b_ih and b_hh are added behind the last MFMA, as rdv_policy_mlp.h adds its biases.
#pragma once

#include "rdv_policy_mlp.h"

namespace rdv {

constexpr int kLstmMaxH = 256;
inline bool lstm_hidden_ok(int H) { return H == 32 || H == 64 || H == 128 || H == 256; }

// The handle's block: [trunk block | cell block].  The trunk block has rdv_policy_mlp.h's layout (header words, layer records, exp(log_std),
// log_std, 64 zeros, fragments, biases) with layer 0 = [hidden[0], H] in natural k order over H / 16 k-steps; header word 4 = H, word 5 =
// float offset of the cell block (a multiple of 4).  Cell block: floats 0..3 = inverse accumulator scale 2^-(10 + s) (float), H (int), 0, 0;
// from float 4 the 2 x 4 H / 32 x (2 + H / 16) fragments [term][tile = q H / 32 + j][ks] (k-steps 0, 1: the 17 inputs, then h); then
// b_ih and b_hh, each [tile][lane half][16] in accumulator order, times the accumulator's scale.
constexpr int kLstmCellHdr = 4;
inline int lstm_cell_tiles(int H) { return 4 * (H / 32); }
inline int lstm_cell_ksteps(int H) { return 2 + H / 16; }
inline size_t lstm_cell_floats(int H) {
  return (size_t)kLstmCellHdr + (size_t)2 * lstm_cell_tiles(H) * lstm_cell_ksteps(H) * (kPolFragBytes / 4) + (size_t)2 * lstm_cell_tiles(H) * 32;
}

// Host: the handle's block from torch's arrays (nn.LSTM: w_ih [4H, 17], w_hh [4H, H], b_ih, b_hh [4H], gate order i, f, g, o; the
// trunk's nn.Linear layers [out, in], hidden layers first, the head last: layer 0 [hidden[0], H]).  `trunk` and H are checked by the caller.
inline void pack_lstm_weights(int H, const RdvMlpSpec& trunk, int out_dim, const float* w_ih, const float* w_hh, const float* b_ih,
                              const float* b_hh, const float* const* weights, const float* const* biases, const float* log_std,
                              std::vector<float>& packed) {
  // ---- the trunk: pack_mlp_weights' block with another first layer
  const int L = trunk.n_hidden;
  int frag0[kMlpLayers], mt_n[kMlpLayers], ks_n[kMlpLayers], in_w[kMlpLayers], out_w[kMlpLayers], frags_total = 0, tiles_total = 0;
  for (int l = 0; l <= L; ++l) {
    in_w[l] = l == 0 ? H : trunk.hidden[l - 1];
    out_w[l] = l < L ? trunk.hidden[l] : out_dim;
    mt_n[l] = l < L ? mlp_tiles(out_w[l]) : 1;
    ks_n[l] = l == 0 ? H / 16 : mlp_ksteps(in_w[l]);
    frag0[l] = frags_total;
    frags_total += 2 * mt_n[l] * ks_n[l];
    tiles_total += mt_n[l];
  }
  const int bias0 = kMlpHdr + frags_total * (kPolFragBytes / 4);
  const int trunk_total = bias0 + tiles_total * 32;                      // a multiple of 4
  packed.assign((size_t)trunk_total + lstm_cell_floats(H), 0.0f);
  int32_t* hdr = reinterpret_cast<int32_t*>(packed.data());
  hdr[0] = L; hdr[1] = trunk.activation; hdr[2] = out_dim; hdr[3] = trunk_total; hdr[4] = H; hdr[5] = trunk_total;
  uint16_t* frags = reinterpret_cast<uint16_t*>(packed.data() + kMlpHdr);
  int bias_at = bias0;
  for (int l = 0; l <= L; ++l) {
    const float* wl = weights[l];
    const int sft = pol_layer_shift(wl, out_w[l] * in_w[l]);
    for (int lane = 0; lane < 64; ++lane) {
      const int r = lane & 31, h = lane >> 5;
      for (int j = 0; j < 8; ++j)
        for (int mt = 0; mt < mt_n[l]; ++mt)
          for (int ks = 0; ks < ks_n[l]; ++ks) {
            // layer 0: natural k order (its B operand is read from the state); later layers: the k order of an accumulator tile
            const int k = l == 0 ? 16 * ks + 8 * h + j : 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
            const int row = 32 * mt + r;
            pol_put(frags, frag0[l], mt_n[l], ks_n[l], mt, ks, lane, j, (row < out_w[l] && k < in_w[l]) ? wl[row * in_w[l] + k] : 0.0f, sft);
          }
    }
    const float acc = std::ldexp(1.0f, kPolXShift + sft);
    for (int mt = 0; mt < mt_n[l]; ++mt)
      for (int h = 0; h < 2; ++h)
        for (int e = 0; e < 16; ++e) {
          const int row = 32 * mt + (e & 3) + 8 * (e >> 2) + 4 * h;
          packed[(size_t)(bias_at + (mt * 2 + h) * 16 + e)] = row < out_w[l] ? biases[l][row] * acc : 0.0f;
        }
    int32_t* rec = hdr + kMlpRec + kMlpRecStride * l;
    rec[0] = frag0[l]; rec[1] = bias_at; rec[2] = mt_n[l]; rec[3] = ks_n[l];
    packed[(size_t)(kMlpRec + kMlpRecStride * l + 4)] = 1.0f / acc;
    bias_at += mt_n[l] * 32;
  }
  if (log_std) for (int j = 0; j < out_dim; ++j) { packed[kMlpStd + j] = std::exp(log_std[j]); packed[kMlpStd + 8 + j] = log_std[j]; }

  // ---- the cell: [W_ih | W_hh] as ONE matrix of 4H rows over 32 (17 used) + H columns, one scale
  float* cell = packed.data() + trunk_total;
  const int tiles = lstm_cell_tiles(H), KS = lstm_cell_ksteps(H);
  const int s_ih = pol_layer_shift(w_ih, 4 * H * kPolIn), s_hh = pol_layer_shift(w_hh, 4 * H * H);
  const int sft = s_ih < s_hh ? s_ih : s_hh;
  const float acc = std::ldexp(1.0f, kPolXShift + sft);
  cell[0] = 1.0f / acc;
  reinterpret_cast<int32_t*>(cell)[1] = H;
  uint16_t* cfrags = reinterpret_cast<uint16_t*>(cell + kLstmCellHdr);
  for (int lane = 0; lane < 64; ++lane) {
    const int r = lane & 31, h = lane >> 5;
    for (int j = 0; j < 8; ++j)
      for (int t = 0; t < tiles; ++t) {
        const int row = (t / (H / 32)) * H + 32 * (t % (H / 32)) + r;     // gate q = t / (H / 32), units 32 j .. of it
        for (int ks = 0; ks < KS; ++ks) {
          const int k = 16 * (ks < 2 ? ks : ks - 2) + 8 * h + j;
          const float wv = ks < 2 ? (k < kPolIn ? w_ih[row * kPolIn + k] : 0.0f) : w_hh[(size_t)row * H + k];
          pol_put(cfrags, 0, tiles, KS, t, ks, lane, j, wv, sft);
        }
      }
  }
  float* cb = cell + kLstmCellHdr + (size_t)2 * tiles * KS * (kPolFragBytes / 4);
  for (int t = 0; t < tiles; ++t)
    for (int h = 0; h < 2; ++h)
      for (int e = 0; e < 16; ++e) {
        const int row = (t / (H / 32)) * H + 32 * (t % (H / 32)) + (e & 3) + 8 * (e >> 2) + 4 * h;
        cb[(t * 2 + h) * 16 + e] = b_ih[row] * acc;
        cb[(size_t)tiles * 32 + (t * 2 + h) * 16 + e] = b_hh[row] * acc;
      }
}

// The launches (rdv_policy_lstm.hip).  `W`: the handle's block on the device.  start: u8 [n] or nullptr (no episode starts).
// h, c: the state; h_next: where the cell kernel leaves h'; c_out: c (a committing call) or a scratch buffer.
// tile_member: nullptr for one network (the block at W), or a recurrent set's tile table (device, one member index per 256 rows): the
// set forms of the kernels, each workgroup reading the block at W + member * block_floats.
void lstm_launch_cell(int H, const float* W, int block_floats, const int32_t* tile_member, const float* obs, const uint8_t* start, const float* h,
                      const float* c, float* h_next, float* c_out, int64_t n, hipStream_t s);
// h_commit: the state's h when the call commits (the rows of h_next are copied there), nullptr otherwise
void lstm_launch_trunk(int activation, bool critic, const float* W, int block_floats, const int32_t* tile_member, const float* h_next, float* h_commit,
                       float* out, int64_t n, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions,
                       float* log_prob, hipStream_t s);
// A recurrent set's last kernel argument (include/rdv.h, "Recurrent policy sets"): P blocks of block_floats floats back to back at W, and
// the member that owns each 256-row tile.  A block is self-describing (header words 4 and 5 are relative to it) and block_floats is a
// multiple of 4, so every 16-byte fragment read stays aligned.
struct LstmSetBlocks {
  const int32_t* tile_member;
  int block_floats;
};
// rows of h and c whose mask byte is not 0 (mask nullptr: every row) <- 0
void lstm_launch_reset(float* h, float* c, const uint8_t* mask, int64_t n, int H, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------- device
// The B fragments (two fp16 terms) of one k-step of h for this lane's env: 8 floats of its state row (nullptr: a row beyond n, or an
// episode start — zeros), times 2^10, clamped to +-63; `keep` receives the 8 floats as read (the trunk kernel commits them).
__device__ __forceinline__ void lstm_h_frag(const float* row8, f16x8 (&b)[2], pol_f4 (&keep)[2]) {
  constexpr float xs = (float)(1 << kPolXShift), xmax = 63.0f * xs;
  keep[0] = pol_f4{0.0f, 0.0f, 0.0f, 0.0f}; keep[1] = keep[0];
  if (row8) { keep[0] = *reinterpret_cast<const pol_f4*>(row8); keep[1] = *reinterpret_cast<const pol_f4*>(row8 + 4); }
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = keep[j >> 2][j & 3];
    const float cl = __builtin_amdgcn_fmed3f(v * xs, -xmax, xmax);
    x[j] = v != v ? v : cl;                                              // NaN stays NaN
  }
  split2(x, b);
}

#ifdef RDV_LSTM_KERNELS   // (rdv_policy_lstm.hip alone takes the kernels; the other units take the packing, the launches and lstm_h_frag)
// The set forms of the two kernels are the same templates with ONE more argument, a LstmSetBlocks: lstm_cell_kernel<H, LstmSetBlocks> and
// lstm_trunk_kernel<ACT, CRITIC, LstmSetBlocks>.  A workgroup owns 256 consecutive rows, which never span two members (every size but the
// last is a multiple of 256), and reads its member's block at W + tile_member[blockIdx.x] * block_floats: one wave-uniform load more, no
// barrier, no LDS hand-off, everything behind it the same device code — so row i of member g gets bit for bit what the plain kernel gives
// a stand-alone handle of that member.  The plain forms (an empty pack) take no such argument and compile to what they were.
__device__ __forceinline__ const float* lstm_member_block(const float* W, const LstmSetBlocks& set) {
  return W + (size_t)set.tile_member[blockIdx.x] * (size_t)set.block_floats;
}

// One call of the cell for the wave's 32 envs.  512 threads = 8 waves = 256 envs per workgroup, as the actor kernels.
template <int H, class... SET>
__global__ __launch_bounds__(kPolBlock) void lstm_cell_kernel(const float* __restrict__ W, const float* __restrict__ obs,
                                                              const uint8_t* __restrict__ start, const float* __restrict__ h_in,
                                                              const float* c_in, float* __restrict__ h_next,
                                                              float* c_out /* = c_in when the call commits */, int64_t n, SET... set) {
  if constexpr (sizeof...(SET) != 0) W = lstm_member_block(W, set...);
  __shared__ __attribute__((aligned(16))) float stage[(kPolBlock / 64) * kPolObsStage];
  constexpr int NB = H / 32, TILES = 4 * NB, KS = 2 + H / 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  float* rows = stage + wv * kPolObsStage;
  const int64_t wave_base = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_base) < kPolWaveEnvs ? (n - wave_base) : kPolWaveEnvs;
  if (nrows <= 0) return;                                                // (no workgroup barrier in this kernel)
  stage_obs_rows(obs, wave_base, nrows, rows, lane);
  wave_fence();
  const float* cell = W + reinterpret_cast<const int32_t*>(W)[5];
  const float inv = cell[0];
  const f16x8* wf = reinterpret_cast<const f16x8*>(cell + kLstmCellHdr) + lane;
  const float* bih = cell + kLstmCellHdr + 2 * TILES * KS * (kPolFragBytes / 4);
  const float* bhh = bih + TILES * 32;
  const bool live = r < nrows;
  const int64_t row = wave_base + r;
  const bool fresh = live && start && start[row] != 0;                   // (1 - s) h, (1 - s) c
  const float* hrow = (live && !fresh) ? h_in + row * H + 8 * hh : nullptr;
  const float* crow = (live && !fresh) ? c_in + row * H + 4 * hh : nullptr;

  f16x8 xb[2][2];
  actor_inputs(rows, lane, xb);
  const float ksig = mlp_act_const<RDV_ACT_SIGMOID>(inv), ktanh = mlp_act_const<RDV_ACT_TANH>(inv);
  constexpr float down = 1.0f / (float)(1 << kPolXShift);
#pragma unroll 1
  for (int jb = 0; jb < NB; ++jb) {
    f32x16 d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = (f32x16)(0.0f);
    auto step = [&](int ks, const f16x8 (&b)[2]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f16x8 a[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = wf[(size_t)((t * TILES + q * NB + jb) * KS + ks) * 64];
        d[q] = mfma3(a, b, d[q]);
      }
    };
    step(0, xb[0]);
    step(1, xb[1]);
#pragma unroll 2
    for (int ks = 0; ks < H / 16; ++ks) {
      f16x8 hb[2];
      pol_f4 keep[2];
      lstm_h_frag(hrow ? hrow + 16 * ks : nullptr, hb, keep);
      step(2 + ks, hb);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mlp_add_bias(d[q], bih + ((q * NB + jb) * 2 + hh) * 16);
      mlp_add_bias(d[q], bhh + ((q * NB + jb) * 2 + hh) * 16);
    }
    // the cell update on the accumulators: register e of lane half hh is unit 32 jb + (e & 3) + 8 (e >> 2) + 4 hh
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      pol_f4 c = {0.0f, 0.0f, 0.0f, 0.0f};
      if (crow) c = *reinterpret_cast<const pol_f4*>(crow + 32 * jb + 8 * e4);
      pol_f4 cn, hn;
#pragma unroll
      for (int p = 0; p < 4; p += 2) {
        const int e = 4 * e4 + p;
        float i0, i1, f0, f1, g0, g1, o0, o1, t0, t1;                    // activations leave times 2^10
        mlp_act2<RDV_ACT_SIGMOID>(d[0][e], d[0][e + 1], ksig, i0, i1);
        mlp_act2<RDV_ACT_SIGMOID>(d[1][e], d[1][e + 1], ksig, f0, f1);
        tanh2_f32(d[2][e], d[2][e + 1], ktanh, g0, g1);
        mlp_act2<RDV_ACT_SIGMOID>(d[3][e], d[3][e + 1], ksig, o0, o1);
        cn[p] = fmaf(f0 * down, c[p], (i0 * down) * (g0 * down));
        cn[p + 1] = fmaf(f1 * down, c[p + 1], (i1 * down) * (g1 * down));
        tanh2_f32(cn[p], cn[p + 1], 2.8853900817779268f, t0, t1);
        hn[p] = (o0 * down) * (t0 * down);
        hn[p + 1] = (o1 * down) * (t1 * down);
      }
      if (live) {
        const int64_t at = row * H + 32 * jb + 8 * e4 + 4 * hh;
        *reinterpret_cast<pol_f4*>(c_out + at) = cn;
        *reinterpret_cast<pol_f4*>(h_next + at) = hn;
      }
    }
  }
}

// first trunk layer: MT tiles over the H / 16 k-steps of h' (read from h_next, committed to h when asked) -> the B fragments of layer 1
template <int ACT, int MT>
__device__ __forceinline__ void lstm_trunk_first(const float* wf, int frag0, int KS, const float* biasp, float k, int lane, const float* hrow,
                                                 float* hdst, f16x8 (&x)[4][2]) {
  f32x16 d[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) d[mt] = (f32x16)(0.0f);
  const f16x8* w8 = reinterpret_cast<const f16x8*>(wf) + lane;
  for (int ks = 0; ks < KS; ++ks) {
    f16x8 hb[2];
    pol_f4 keep[2];
    lstm_h_frag(hrow ? hrow + 16 * ks : nullptr, hb, keep);
    if (hdst) {
      *reinterpret_cast<pol_f4*>(hdst + 16 * ks) = keep[0];
      *reinterpret_cast<pol_f4*>(hdst + 16 * ks + 4) = keep[1];
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      f16x8 a[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) a[t] = w8[(size_t)(frag0 + (t * MT + mt) * KS + ks) * 64];
      d[mt] = mfma3(a, hb, d[mt]);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mlp_add_bias(d[mt], biasp + (mt * 2 + (lane >> 5)) * 16);
    mlp_activate<ACT>(d[mt], k, x[2 * mt], x[2 * mt + 1]);
  }
}

// The trunk and the head for the wave's 32 envs; CRITIC: out = values [n], otherwise actions [n, 6] (and raw_actions / log_prob).
// (the noise of row i is keyed by env_id_offset + i, i counted over all rows: in a set, a stand-alone member's env_id_offset + start_g + its row)
template <int ACT, bool CRITIC, class... SET>
__global__ __launch_bounds__(kPolBlock) void lstm_trunk_kernel(const float* __restrict__ W, const float* __restrict__ h_next, float* __restrict__ h_commit,
                                                               float* __restrict__ out, int64_t n, int deterministic, uint64_t seed,
                                                               uint64_t counter, uint64_t env_id_offset, float* __restrict__ raw_actions,
                                                               float* __restrict__ log_prob, SET... set) {
  if constexpr (sizeof...(SET) != 0) W = lstm_member_block(W, set...);
  __shared__ __attribute__((aligned(16))) float astage[(kPolBlock / 64) * kPolActStage];
  const int32_t* Hd = reinterpret_cast<const int32_t*>(W);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  float* arows = astage + wv * kPolActStage;
  const int64_t wave_base = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_base) < kPolWaveEnvs ? (n - wave_base) : kPolWaveEnvs;
  if (nrows <= 0) return;
  const int L = Hd[0], Hn = Hd[4];
  const float* wf = W + kMlpHdr;
  const float* zerop = W + kMlpZero;
  const bool live = r < nrows;
  const int64_t row = wave_base + r;
  const float* hrow = live ? h_next + row * Hn + 8 * hh : nullptr;
  float* hdst = (live && h_commit) ? h_commit + row * Hn + 8 * hh : nullptr;
  f16x8 x[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) { x[i][0] = (f16x8)(0); x[i][1] = (f16x8)(0); }
  {
    const int32_t* rec = Hd + kMlpRec;
    const float k = mlp_act_const<ACT>(__int_as_float(rec[4]));
    if (rec[2] == 2) lstm_trunk_first<ACT, 2>(wf, rec[0], rec[3], W + rec[1], k, lane, hrow, hdst, x);
    else lstm_trunk_first<ACT, 1>(wf, rec[0], rec[3], W + rec[1], k, lane, hrow, hdst, x);
  }
  // layers 1 .. L-1 and the head: the wave-uniform switch of mlp_means over the (MT, KS) shapes
#pragma nounroll
  for (int l = 1; l < L; ++l) {
    const int32_t* rec = Hd + kMlpRec + kMlpRecStride * l;
    const int frag0 = rec[0];
    const float* biasp = W + rec[1];
    const float k = mlp_act_const<ACT>(__int_as_float(rec[4]));
    switch (rec[2] * 8 + rec[3]) {
      case 8 + 1: mlp_hidden<ACT, 1, 1>(wf, zerop, frag0, biasp, k, lane, x); break;
      case 8 + 2: mlp_hidden<ACT, 1, 2>(wf, zerop, frag0, biasp, k, lane, x); break;
      case 8 + 4: mlp_hidden<ACT, 1, 4>(wf, zerop, frag0, biasp, k, lane, x); break;
      case 16 + 1: mlp_hidden<ACT, 2, 1>(wf, zerop, frag0, biasp, k, lane, x); break;
      case 16 + 2: mlp_hidden<ACT, 2, 2>(wf, zerop, frag0, biasp, k, lane, x); break;
      default: mlp_hidden<ACT, 2, 4>(wf, zerop, frag0, biasp, k, lane, x); break;
    }
  }
  float a[4];
  {
    const int32_t* rec = Hd + kMlpRec + kMlpRecStride * L;
    const float inv = __int_as_float(rec[4]);
    switch (rec[3]) {
      case 1: mlp_head<1>(wf, zerop, rec[0], W + rec[1], inv, lane, x, a); break;
      case 2: mlp_head<2>(wf, zerop, rec[0], W + rec[1], inv, lane, x, a); break;
      default: mlp_head<4>(wf, zerop, rec[0], W + rec[1], inv, lane, x, a); break;
    }
  }
  if (CRITIC) {
    if (lane < nrows) out[wave_base + lane] = a[0];
  } else {
    actor_outputs(W + kMlpStd, lane, wave_base, nrows, deterministic, seed, counter, env_id_offset, a, arows, out, raw_actions, log_prob);
  }
}

__global__ __launch_bounds__(256) void lstm_reset_kernel(float* __restrict__ h, float* __restrict__ c, const uint8_t* __restrict__ mask, int64_t n, int H) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;             // one float4 of a row
  const int per_row = H / 4;
  const int64_t row = q / per_row;
  if (row >= n || (mask && mask[row] == 0)) return;
  reinterpret_cast<pol_f4*>(h)[q] = pol_f4{0.0f, 0.0f, 0.0f, 0.0f};
  reinterpret_cast<pol_f4*>(c)[q] = pol_f4{0.0f, 0.0f, 0.0f, 0.0f};
}
#endif   // RDV_LSTM_KERNELS

}  // namespace rdv

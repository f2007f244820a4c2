// rdv_ppo_lstm.hip — the kernels of rdv_ppo_lstm.h and their launch, in a translation unit of its own (the objects of the other units do
// not change when it does).  The exported rdv_lstm_ppo_* entry points are in rdv_policy_host.hip.  The forward replay is
// lstm_cell_keep_kernel below, lstm_cell_kernel's body restated with the gates kept; the trunk's layers 1 .. L, the loss terms and the weight-gradient contraction of the
// trunk are the functions of rdv_ppo_mlp.h and rdv_ppo_ops.h.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_ppo_lstm.h"

#include <type_traits>

namespace rdv {

// ---- the set form: what every SET kernel derives of its member from the by-value arguments (rdv_ppo_lstm.h, "the set form")
// member g's piece of the workspace: where it starts and, for net k (0 actor, 1 critic), the stand-alone layout of (T, B_g)
__device__ __forceinline__ float* lstm_ppo_member_ws(const LstmPpoSetCommon& c, int g, int k, int64_t B, LstmPpoHeadWs& hd, LstmPpoNetWs& o) {
  hd = lstm_ppo_head_layout(c.T, B);
  const int64_t end0 = lstm_ppo_net_layout(c.d, 0, c.T, B, hd.end, o);
  if (k == 1) lstm_ppo_net_layout(c.d, 1, c.T, B, end0, o);
  return c.ws + c.table.ws[g];
}
__device__ __forceinline__ const float* lstm_ppo_member_block(const LstmPpoSetCommon& c, int g, int k) {
  return c.block[k] + (size_t)g * c.block_floats[k];
}

// a value as an MFMA operand reads it: times 2^10, clamped to +-63, a NaN kept (actor_inputs, lstm_h_frag)
__device__ __forceinline__ float lstm_ppo_operand(float v) {
  constexpr float xs = (float)(1 << kPolXShift), xmax = 63.0f * xs;
  const float cl = __builtin_amdgcn_fmed3f(v * xs, -xmax, xmax);
  return v != v ? v : cl;
}

// ---- 0. the minibatch's columns gathered (blockIdx.y: 0 observations, 1 episode starts, 2 .. 5 the four state0 arrays)
struct LstmPpoGatherArgs {
  const float* obs;
  const uint8_t* done;
  const float* st[4];
  const int64_t* envs;
  float* obs_g;
  uint8_t* start_g;
  float* st_g[4];
  int64_t N, B, T, obs_stride;
  int32_t Ha, Hc;
};
// the set form's arguments: `g` holds the set-wide values (envs: all members'; obs_g, start_g, st_g, B, obs_stride unused)
struct LstmPpoSetGatherArgs {
  LstmPpoGatherArgs g;
  LstmPpoSetCommon c;
};
static_assert(sizeof(LstmPpoSetGatherArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <bool SET> using LstmPpoGatherKernelArgs = std::conditional_t<SET, LstmPpoSetGatherArgs, LstmPpoGatherArgs>;
__device__ __forceinline__ const LstmPpoGatherArgs& lstm_ppo_gather_args(const LstmPpoGatherArgs& S, const LstmPpoGatherArgs&) { return S; }
__device__ __forceinline__ const LstmPpoGatherArgs& lstm_ppo_gather_args(const LstmPpoSetGatherArgs&, const LstmPpoGatherArgs& M) { return M; }
// SET = false: the kernel of rdv_lstm_ppo_loss_grad.  SET = true: workgroup (x, y, z) is workgroup (x, y) of member z's stand-alone launch.
template <bool SET>
__global__ __launch_bounds__(256) void lstm_ppo_gather_kernel(const LstmPpoGatherKernelArgs<SET> S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  [[maybe_unused]] LstmPpoGatherArgs M;                   // SET: the member's scalars (its two arrays of pointers are not read: they
  [[maybe_unused]] float* st_set = nullptr;               // stay in the kernel arguments; st_set: where state0 array y - 2 goes)
  if constexpr (SET) {
    const int g = blockIdx.z;
    const int64_t B = S.c.table.count[g];
    if (B == 0) return;
    LstmPpoHeadWs hd;
    LstmPpoNetWs o;
    float* ws = lstm_ppo_member_ws(S.c, g, y >= 4 ? 1 : 0, B, hd, o);
    M.obs = S.g.obs; M.done = S.g.done; M.N = S.g.N; M.T = S.g.T;
    M.envs = S.g.envs + S.c.table.off[g];
    M.B = B;
    M.obs_stride = hd.obs_stride;
    M.obs_g = ws + hd.obs;
    M.start_g = reinterpret_cast<uint8_t*>(ws + hd.start);
    st_set = ws + ((y & 1) ? o.c0 : o.h0);
  }
  const LstmPpoGatherArgs& A = lstm_ppo_gather_args(S, M);
  if (y == 0) {
    const int64_t per = A.B * kPolIn;
    if (i >= A.T * per) return;
    const int64_t t = i / per, rem = i - t * per, b = rem / kPolIn, f = rem - b * kPolIn;
    const int64_t env = A.envs ? A.envs[b] : b;
    A.obs_g[t * A.obs_stride + rem] = A.obs[(t * A.N + env) * kPolIn + f];
  } else if (y == 1) {
    if (i >= A.T * A.B) return;
    const int64_t t = i / A.B, b = i - t * A.B;
    const int64_t env = A.envs ? A.envs[b] : b;
    A.start_g[i] = t == 0 ? (uint8_t)0 : (uint8_t)(A.done[(t - 1) * A.N + env] != 0);
  } else {
    const int k = y - 2;
    int H;
    if constexpr (SET) H = k < 2 ? S.g.Ha : S.g.Hc; else H = k < 2 ? S.Ha : S.Hc;   // (a value of the kernel arguments themselves, as it was)
    if (i >= A.B * H) return;
    const int64_t b = i / H, u = i - b * H;
    const int64_t env = A.envs ? A.envs[b] : b;
    if constexpr (SET) st_set[i] = S.g.st[k][env * H + u];
    else A.st_g[k][i] = A.st[k][env * H + u];
  }
}

// ---- 0. the transposed fragments of W_hh and of the trunk's layer 0, copied term by term from the forward block (blockIdx.y: the net)
//   W_hh^T, fragment (term, mt, ks) of 2 x H / 32 x 4 H / 16, lane (r, h), element j:  W_hh[R][C], R = 16 ks + 8 h + j (gate row, natural
//   order, as da lies in memory), C = 32 mt + r; the forward keeps it in tile (R / H) H / 32 + (R % H) / 32, k-step 2 + C / 16.
//   W_0^T, fragment (term, mt, ks) of 2 x H / 32 x k-steps of hidden[0], lane (r, h), element j:  W_0[o][i], o = perm(ks, h, j) (delta_0 is
//   an accumulator tile), i = 32 mt + r; the forward keeps it in tile o >> 5, k-step i / 16 (natural k order), or has no such row: zero.
struct LstmPpoTransposeArgs {
  const float* block[2];
  float* whht[2];
  float* w0t[2];
};
// SET = false: the kernel of rdv_lstm_ppo_loss_grad.  SET = true (the arguments: LstmPpoSetCommon alone): member blockIdx.z's block of the
// sets' allocations -> its piece of the workspace; a member without columns is skipped.
static_assert(sizeof(LstmPpoSetCommon) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <bool SET>
__global__ __launch_bounds__(512) void lstm_ppo_transpose_kernel(const std::conditional_t<SET, LstmPpoSetCommon, LstmPpoTransposeArgs> A) {
  const int net = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  [[maybe_unused]] float *whht_set = nullptr, *w0t_set = nullptr;
  if constexpr (SET) {
    const int g = blockIdx.z;
    const int64_t B = A.table.count[g];
    if (B == 0) return;
    LstmPpoHeadWs hd;
    LstmPpoNetWs o;
    float* ws = lstm_ppo_member_ws(A, g, net, B, hd, o);
    whht_set = ws + o.whht;
    w0t_set = ws + o.w0t;
  }
  auto whht = [&]() -> float* { if constexpr (SET) return whht_set; else return A.whht[net]; };
  auto w0t = [&]() -> float* { if constexpr (SET) return w0t_set; else return A.w0t[net]; };
  const float* block;
  if constexpr (SET) block = lstm_ppo_member_block(A, blockIdx.z, net); else block = A.block[net];
  const int32_t* Hd = reinterpret_cast<const int32_t*>(block);
  const int H = Hd[4], NB = H / 32, KSB = H / 4;
  const int KSd = Hd[kMlpRec + kMlpRecStride + 3];                        // the k-steps of layer 1's input: hidden[0] / 16
  const int nW = 2 * NB * KSB, n0 = 2 * NB * KSd;
  const int lane = t >> 3, j = t & 7, r = lane & 31, h = lane >> 5;
  if (b < nW) {
    const int term = b / (NB * KSB), mt = (b / KSB) % NB, ks = b % KSB;
    const int R = 16 * ks + 8 * h + j, C = 32 * mt + r;
    const int tile = (R / H) * NB + (R % H) / 32, rp = (R % H) % 32, ksp = 2 + C / 16, hp = (C % 16) / 8, jp = C % 8;
    const int TILES = 4 * NB, KS = 2 + H / 16;
    const uint16_t* src = reinterpret_cast<const uint16_t*>(block + Hd[5] + kLstmCellHdr);
    reinterpret_cast<uint16_t*>(whht())[((size_t)b * 64 + lane) * 8 + j] =
        src[((size_t)((term * TILES + tile) * KS + ksp) * 64 + (size_t)(rp + 32 * hp)) * 8 + jp];
  } else if (b - nW < n0) {
    const int b2 = b - nW;
    const int term = b2 / (NB * KSd), mt = (b2 / KSd) % NB, ks = b2 % KSd;
    const int o = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3), i = 32 * mt + r;
    const int32_t* rec = Hd + kMlpRec;
    const int frag0 = rec[0], MT0 = rec[2], KS0 = rec[3];
    uint16_t v = 0;
    if ((o >> 5) < MT0) {
      const uint16_t* src = reinterpret_cast<const uint16_t*>(block + kMlpHdr);
      v = src[((size_t)(frag0 + (term * MT0 + (o >> 5)) * KS0 + i / 16) * 64 + (size_t)((o & 31) + 32 * ((i % 16) / 8))) * 8 + (i % 8)];
    }
    reinterpret_cast<uint16_t*>(w0t())[((size_t)b2 * 64 + lane) * 8 + j] = v;
  }
}

// One call of the cell for the wave's 32 envs: the body of lstm_cell_kernel (rdv_policy_lstm.h), statement for statement, with the gate
// activations i, f, g, o as the cell update uses them kept -> gates [n, 4 H] (row-major, gate q of unit u at q H + u).  A restatement and not
// a shared function: lstm_cell_kernel's instruction stream is pinned to its recorded digest (profiles/lstm_sets_isa_diff.md,
// tests/test_lstm_policy_sets.py), and calling a common body from it changes the register allocation; every floating-point operation is
// element-wise per env column and written as there, and tests/test_gpu_ppo_lstm_grad.py holds the replayed values to the rollout's bits
// for every H.  `stage`: the workgroup's LDS observation rows.
template <int H, bool KEEP = true>
__device__ __forceinline__ void lstm_cell_rows(const float* W, const float* obs, const uint8_t* start, const float* h_in, const float* c_in,
                                               float* h_next, float* c_out, float* gates, int64_t n, float* stage) {
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
      [[maybe_unused]] pol_f4 kept[4];
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
        if constexpr (KEEP) {
          kept[0][p] = i0 * down; kept[0][p + 1] = i1 * down; kept[1][p] = f0 * down; kept[1][p + 1] = f1 * down;
          kept[2][p] = g0 * down; kept[2][p + 1] = g1 * down; kept[3][p] = o0 * down; kept[3][p + 1] = o1 * down;
        }
      }
      if (live) {
        const int64_t at = row * H + 32 * jb + 8 * e4 + 4 * hh;
        *reinterpret_cast<pol_f4*>(c_out + at) = cn;
        *reinterpret_cast<pol_f4*>(h_next + at) = hn;
        if constexpr (KEEP) {
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<pol_f4*>(gates + row * (4 * H) + q * H + 32 * jb + 8 * e4 + 4 * hh) = kept[q];
        }
      }
    }
  }
}


// ---- 1. one step of the forward replay: lstm_cell_rows on the gathered rows of step t
template <int H>
__global__ __launch_bounds__(kPolBlock) void lstm_cell_keep_kernel(const float* __restrict__ W, const float* __restrict__ obs,
                                                                   const uint8_t* __restrict__ start, const float* __restrict__ h_in,
                                                                   const float* __restrict__ c_in, float* __restrict__ h_next,
                                                                   float* __restrict__ c_out, float* __restrict__ gates, int64_t n) {
  __shared__ __attribute__((aligned(16))) float stage[(kPolBlock / 64) * kPolObsStage];
  lstm_cell_rows<H, true>(W, obs, start, h_in, c_in, h_next, c_out, gates, n, stage);
}
// the set form: workgroup (x, y) is workgroup x of member y's stand-alone launch of step t for net k — lstm_cell_rows on the pointers
// that lstm_ppo_launch passes, derived from the member's piece (the plain kernel keeps its nine arguments and so its code).  A wave
// beyond the member's columns returns in lstm_cell_rows, which has no workgroup barrier.
struct LstmPpoSetCellArgs {
  LstmPpoSetCommon c;
  int32_t k, t;
};
static_assert(sizeof(LstmPpoSetCellArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <int H>
__global__ __launch_bounds__(kPolBlock) void lstm_cell_keep_set_kernel(const LstmPpoSetCellArgs S) {
  __shared__ __attribute__((aligned(16))) float stage[(kPolBlock / 64) * kPolObsStage];
  const int g = blockIdx.y;
  const int64_t B = S.c.table.count[g];
  if ((int64_t)blockIdx.x * kPolBlockEnvs >= B) return;
  LstmPpoHeadWs hd;
  LstmPpoNetWs o;
  float* ws = lstm_ppo_member_ws(S.c, g, S.k, B, hd, o);
  const int64_t t = S.t;
  const float* h_in = t == 0 ? ws + o.h0 : ws + o.hs + (t - 1) * B * H;
  const float* c_in = t == 0 ? ws + o.c0 : ws + o.cs + (t - 1) * B * H;
  const uint8_t* start = t == 0 ? nullptr : reinterpret_cast<const uint8_t*>(ws + hd.start) + t * B;
  lstm_cell_rows<H, true>(lstm_ppo_member_block(S.c, g, S.k), ws + hd.obs + t * hd.obs_stride, start, h_in, c_in, ws + o.hs + t * B * H,
                          ws + o.cs + t * B * H, ws + o.gates + t * B * 4 * H, B, stage);
}

// ---- 2. the trunk over all T B rows
struct LstmPpoTrunkArgs {
  const float *block, *bwd, *w0t, *hs;   // forward block, the trunk's backward block (layers 1 .. L), W_0^T, h_t [n, H]
  PpoRowArgs rows;                       // the [T, N] columns (obs and indices unused), n = T B
  const int64_t* envs;                   // nullable
  int64_t N, B;
  float *parts, *out, *dh;               // [workgroups][T.part_floats]; nullable [n]; [n, H]
  int32_t H;
  PpoMlpTable T;
};
// The set form's arguments: `net` holds the set-wide values (the [T, N] columns, envs and out: all members'; N, H, T: the one table of
// this net; the other pointers, B and rows.n unused); lstm_ppo_trunk_member derives member blockIdx.y's own WITHOUT the table, which stays
// in the kernel-argument segment (a private copy indexed by the layer would be scratch).  `idle`: workgroup x has no rows of that member
// (it has fewer workgroups than the widest member, or no columns) — workgroup-uniform, taken before the first barrier.
struct LstmPpoSetTrunkArgs {
  LstmPpoTrunkArgs net;
  LstmPpoSetCommon c;
};
static_assert(sizeof(LstmPpoSetTrunkArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
struct LstmPpoTrunkMember {
  const float *block, *bwd, *hs;
  PpoRowArgs rows;
  const int64_t* envs;
  int64_t N, B;
  float *parts, *out;
  int32_t H, k;
  const LstmPpoSetCommon* c;     // (the kernel arguments: W_0^T and dh are derived from them where layer 0's step starts)
};
template <bool SET> using LstmPpoTrunkKernelArgs = std::conditional_t<SET, LstmPpoSetTrunkArgs, LstmPpoTrunkArgs>;
__host__ __device__ __forceinline__ const PpoMlpTable& lstm_ppo_table_of(const LstmPpoTrunkArgs& S) { return S.T; }
__host__ __device__ __forceinline__ const PpoMlpTable& lstm_ppo_table_of(const LstmPpoSetTrunkArgs& S) { return S.net.T; }
template <bool ACTOR, bool SET>
__device__ __forceinline__ decltype(auto) lstm_ppo_trunk_member(const LstmPpoTrunkKernelArgs<SET>& S, bool& idle) {
  if constexpr (SET) {
    constexpr int k = ACTOR ? 0 : 1;
    const int g = blockIdx.y;
    const int64_t B = S.c.table.count[g], n = S.c.T * B, off = S.c.table.off[g];
    idle = (int64_t)blockIdx.x * kPolBlockEnvs >= n;
    LstmPpoHeadWs hd;
    LstmPpoNetWs o;
    float* ws = lstm_ppo_member_ws(S.c, g, k, B, hd, o);
    LstmPpoTrunkMember M;
    M.block = lstm_ppo_member_block(S.c, g, k);
    M.bwd = ws + (size_t)k * kPpoMlpBwdFloats;
    M.hs = ws + o.hs;
    M.rows = S.net.rows;
    M.rows.n = n;
    M.envs = S.net.envs + off;
    M.N = S.net.N;
    M.B = B;
    M.parts = ws + o.tparts;
    M.out = S.net.out ? S.net.out + S.c.T * off : nullptr;
    M.H = S.net.H;
    M.k = k;
    M.c = &S.c;
    return M;
  } else {
    idle = false;
    return (S);                                            // the arguments themselves: the plain kernel is the code it was
  }
}

// lstm_trunk_first of rdv_policy_lstm.h, the same operations in the same order, with the activations of its MT tiles kept
template <int ACT, int MT>
__device__ __forceinline__ void lstm_trunk_first_keep(const float* wf, int frag0, int KS, const float* biasp, float k, int lane, const float* hrow,
                                                      f16x8 (&x)[4][2], float (&hs)[2][16]) {
  f32x16 d[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) d[mt] = (f32x16)(0.0f);
  const f16x8* w8 = reinterpret_cast<const f16x8*>(wf) + lane;
  for (int ks = 0; ks < KS; ++ks) {
    f16x8 hb[2];
    pol_f4 keep[2];
    lstm_h_frag(hrow ? hrow + 16 * ks : nullptr, hb, keep);
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
    ppo_activate_keep<ACT>(d[mt], k, x[2 * mt], x[2 * mt + 1], hs[mt]);
  }
}

// this lane's 16 values of column tile nt of its row of `src` [.., H] as an operand (nullptr: zeros), in accumulator order
__device__ __forceinline__ void lstm_ppo_h_tile(const float* row, int nt, int hh, float (&v)[16]) {
#pragma unroll
  for (int e4 = 0; e4 < 4; ++e4) {
    pol_f4 q = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row) q = *reinterpret_cast<const pol_f4*>(row + 32 * nt + 8 * e4 + 4 * hh);
#pragma unroll
    for (int p = 0; p < 4; ++p) v[4 * e4 + p] = lstm_ppo_operand(q[p]);
  }
}

// W_0^T and dh, which only layer 0's step reads.  The set form derives them HERE from the kernel arguments, behind an opaque copy of the
// member's column count, and not with the member's other pointers ahead of the layers' loop: the actor kernel has no scalar register left
// for two more pointers that live across that loop (they would spill, through a vector register it does not have either, to scratch).
struct LstmPpoFirstPointers { const float* w0t; float* dh; };
__device__ __forceinline__ const LstmPpoTrunkArgs& lstm_ppo_first_pointers(const LstmPpoTrunkArgs& A) { return A; }   // (read where they are used, as they were)
__device__ __forceinline__ LstmPpoFirstPointers lstm_ppo_first_pointers(const LstmPpoTrunkMember& A) {
  const int g = blockIdx.y;
  int64_t B = A.c->table.count[g];
  asm volatile("" : "+s"(B));
  LstmPpoHeadWs hd;
  LstmPpoNetWs o;
  float* ws = lstm_ppo_member_ws(*A.c, g, A.k, B, hd, o);
  return {ws + o.w0t, ws + o.dh};
}

// layer 0 of the trunk: d loss / d h_t = W_0^T delta_0 -> dh; dW_0 = delta_0 h_t^T (two column tiles of h_t at a time) and db_0
template <int KSd, class Member>
__device__ __forceinline__ void lstm_ppo_first_step(const Member& A, const PpoMlpTable& T, float inv_acc, float (&dl)[2][16], bool valid, int64_t m, float* wave_tiles,
                                                    const float* tiles0, int lane, float* part) {
  constexpr int MTd = KSd == 4 ? 2 : 1;
  constexpr float xs = (float)(1 << kPolXShift), inv_xs = 1.0f / xs;
  const int H = A.H, NB = H / 32, hh = lane >> 5;
  const auto& P0 = lstm_ppo_first_pointers(A);
  float S, invS;
  wave_scale(MTd == 2 ? fmaxf(tile_max(dl[0]), tile_max(dl[1])) : tile_max(dl[0]), S, invS);
#pragma unroll
  for (int mt = 0; mt < MTd; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dl[mt][e] *= S;
  {
    f16x8 b[KSd][2];
    if constexpr (KSd == 1) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = dl[0][j];
      split2(x, b[0]);
    } else {
#pragma unroll
      for (int s = 0; s < KSd; ++s) error_frags(dl[s >> 1], s & 1, b[s]);
    }
    const f16x8* w8 = reinterpret_cast<const f16x8*>(P0.w0t) + lane;
    const float un = inv_acc * xs * invS;
#pragma unroll 1
    for (int mt = 0; mt < NB; ++mt) {
      f32x16 pre = (f32x16)(0.0f);
#pragma unroll
      for (int ks = 0; ks < KSd; ++ks) {
        f16x8 a[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = w8[(size_t)((t * NB + mt) * KSd + ks) * 64];
        pre = mfma3(a, b[ks], pre);
      }
      if (valid) {
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
          *reinterpret_cast<pol_f4*>(P0.dh + m * H + 32 * mt + 8 * e4 + 4 * hh) =
              pol_f4{pre[4 * e4] * un, pre[4 * e4 + 1] * un, pre[4 * e4 + 2] * un, pre[4 * e4 + 3] * un};
      }
    }
  }
  _Float16* tb = reinterpret_cast<_Float16*>(wave_tiles);
  const float* hrow = valid ? A.hs + m * H : nullptr;
  const int w_off = T.w_off[0], b_off = T.b_off[0], out_w = T.out_w[0];
#pragma unroll 1
  for (int nt0 = 0; nt0 < NB; nt0 += 2) {
    float hv[16];
    lstm_ppo_h_tile(hrow, nt0, hh, hv);
    stage_tile(tb, hv, lane);
    if (NB > 1) {
      lstm_ppo_h_tile(hrow, nt0 + 1, hh, hv);
      stage_tile(tb + 2 * kPpoTile, hv, lane);
    }
    auto store = [&](int row, int col, float v) {
      if (col >= 0) { if (row < out_w) part[w_off + row * H + 32 * nt0 + col] = v; }
      else if (col == -1 && row < out_w) part[b_off + row] = v;
    };
    if (NB > 1) weight_grads<MTd, 2, 0>(dl, wave_tiles, tiles0, 8, invS * inv_xs, lane, store);
    else weight_grads<MTd, 1, 0>(dl, wave_tiles, tiles0, 8, invS * inv_xs, lane, store);
  }
}

// Eight waves, each 32 rows; trailing waves of the last workgroup have no rows and stay (barriers).
// SET = false: the kernel of rdv_lstm_ppo_loss_grad (profiles/lstm_ppo_set_isa_diff.md).  SET = true: workgroup (x, y) is workgroup x of
// member y's stand-alone launch: the same body on the member's arguments.
template <int ACT, bool ACTOR, bool SET>
__global__ __launch_bounds__(kPolBlock) void lstm_ppo_trunk_kernel(const LstmPpoTrunkKernelArgs<SET> S) {
  bool idle;
  const auto& A = lstm_ppo_trunk_member<ACTOR, SET>(S, idle);
  if (SET && idle) return;
  extern __shared__ __attribute__((aligned(16))) float lstm_ppo_lds[];
  constexpr int nw = kPolBlock / 64;
  const PpoMlpTable& T = lstm_ppo_table_of(S);
  const float* w = A.block;
  const int32_t* Hd = reinterpret_cast<const int32_t*>(A.block);
  const int L = T.L, H = A.H;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  float* tiles0 = lstm_ppo_lds;
  float* wave_tiles = tiles0 + wv * kPpoWaveTiles;
  float* red = tiles0 + nw * kPpoWaveTiles;
  const int64_t wave_base = ((int64_t)blockIdx.x * nw + wv) * kPolWaveEnvs;
  const int64_t left = A.rows.n - wave_base;
  const int nrows = left < 0 ? 0 : (left < kPolWaveEnvs ? (int)left : kPolWaveEnvs);
  const bool valid = r < nrows;
  const int mrow = (int)(wave_base + r);                  // this lane's row (n <= 2^31); addresses are formed where they are used: the
                                                          // backward steps below leave no register for a pointer that lives across them
  float* part = A.parts + (size_t)blockIdx.x * T.part_floats;
  f16x8 x[4][2];
  float hs[2][16], dl[2][16];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) { hs[mt][e] = 0.0f; dl[mt][e] = 0.0f; }

#pragma nounroll
  for (int l = L; l >= 1; --l) {
    // h_l, recomputed: the operations of lstm_trunk_kernel
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i][0] = (f16x8)(0); x[i][1] = (f16x8)(0); }
    {
      const int32_t* rec0 = Hd + kMlpRec;
      const float k0 = mlp_act_const<ACT>(__int_as_float(rec0[4]));
      const float* hrow = valid ? A.hs + (int64_t)mrow * H + 8 * hh : nullptr;
      if (rec0[2] == 2) lstm_trunk_first_keep<ACT, 2>(w + kMlpHdr, rec0[0], rec0[3], w + rec0[1], k0, lane, hrow, x, hs);
      else lstm_trunk_first_keep<ACT, 1>(w + kMlpHdr, rec0[0], rec0[3], w + rec0[1], k0, lane, hrow, x, hs);
    }
    mlp_layers_keep<ACT>(w, Hd, lane, 1, l, x, hs);
    const int32_t* rec = Hd + kMlpRec + kMlpRecStride * l;
    if (l == L) {
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
      int64_t src = 0;                                    // the row of the [T, N] columns: step t, the column's env
      if (valid) {
        const int64_t t = mrow / A.B, b = mrow - t * A.B;
        src = t * A.N + (A.envs ? A.envs[b] : b);
      }
      ppo_loss_terms<ACTOR>(A.rows, w + kMlpStd, w + kMlpStd + 8, mean, valid, src, A.out, (int64_t)mrow, lane, red + wv * 4, d3, ex);
#pragma unroll
      for (int c = 0; c < 4; ++c) { dl[0][c] = d3[c]; dl[0][4 + c] = ex[c]; }
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
    if (l == L) ppo_store_scalar_sums<ACTOR>(red, nw, part + T.part_floats - 4);
  }
  const float inv0 = __int_as_float(Hd[kMlpRec + 4]);
  switch (T.ks[1]) {
    case 1: lstm_ppo_first_step<1>(A, T, inv0, dl, valid, (int64_t)mrow, wave_tiles, tiles0, lane, part); break;
    case 2: lstm_ppo_first_step<2>(A, T, inv0, dl, valid, (int64_t)mrow, wave_tiles, tiles0, lane, part); break;
    default: lstm_ppo_first_step<4>(A, T, inv0, dl, valid, (int64_t)mrow, wave_tiles, tiles0, lane, part); break;
  }
}

// ---- 3. one step of the backward pass through time for the wave's 32 columns (no barrier, no LDS)
struct LstmPpoBpttArgs {
  const float *block, *whht, *cs, *c0, *dh;   // forward block (the accumulator scale), W_hh^T, c_t [n, H], c0_g [B, H], dh(trunk) [n, H]
  float *gates, *dcc, *dscale;                // [n, 4 H]: gates of step t -> da_t; f dc carried [B, H]; the waves' max |da| [T][waves]
  const uint8_t* start;                       // start_g [T][B]
  int64_t B;
  int32_t T, t;
};
// the set form's arguments and member blockIdx.y's own: the arguments lstm_ppo_launch passes for (T, B_g) and the member's piece.  A wave
// beyond the member's columns returns (`nrows <= 0`; the kernel has no barrier).
struct LstmPpoSetBpttArgs {
  LstmPpoSetCommon c;
  int32_t k, t;
};
static_assert(sizeof(LstmPpoSetBpttArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <bool SET> using LstmPpoBpttKernelArgs = std::conditional_t<SET, LstmPpoSetBpttArgs, LstmPpoBpttArgs>;
template <bool SET>
__device__ __forceinline__ decltype(auto) lstm_ppo_bptt_member(const LstmPpoBpttKernelArgs<SET>& S) {
  if constexpr (SET) {
    const int g = blockIdx.y;
    const int64_t B = S.c.table.count[g];
    LstmPpoHeadWs hd;
    LstmPpoNetWs o;
    float* ws = lstm_ppo_member_ws(S.c, g, S.k, B, hd, o);
    const LstmPpoBpttArgs M = {lstm_ppo_member_block(S.c, g, S.k), ws + o.whht, ws + o.cs, ws + o.c0, ws + o.dh, ws + o.gates, ws + o.dcc, ws + o.dscale,
                               reinterpret_cast<const uint8_t*>(ws + hd.start), B, (int32_t)S.c.T, S.t};
    return M;
  } else {
    return (S);                                            // the arguments themselves: the plain kernel is the code it was
  }
}
template <int H, bool SET>
__global__ __launch_bounds__(kPolBlock) void lstm_ppo_bptt_kernel(const LstmPpoBpttKernelArgs<SET> K) {
  const auto& A = lstm_ppo_bptt_member<SET>(K);
  constexpr int NB = H / 32, KSB = H / 4, G = 4 * H;
  constexpr float xs = (float)(1 << kPolXShift), down = 1.0f / xs;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int64_t gw = (int64_t)blockIdx.x * (kPolBlock / 64) + wv, wave_base = gw * kPolWaveEnvs;
  const int64_t nrows = (A.B - wave_base) < kPolWaveEnvs ? (A.B - wave_base) : kPolWaveEnvs;
  if (nrows <= 0) return;
  const int64_t nwaves = (A.B + kPolWaveEnvs - 1) / kPolWaveEnvs;
  const bool live = r < nrows, last = A.t == A.T - 1;
  const int64_t b = wave_base + r, m = (int64_t)A.t * A.B + b;
  const bool flow = !last && live && A.start[m + A.B] == 0;          // done[t] = 0: step t + 1 continues this column's episode
  const bool fresh = A.t > 0 && live && A.start[m] != 0;             // s_t = 1: c_{t-1} entered the cell as zero
  const float inv = (A.block + reinterpret_cast<const int32_t*>(A.block)[5])[0];
  float S = 1.0f, invS = 1.0f;
  if (!last) wave_scale(A.dscale[(int64_t)(A.t + 1) * nwaves + gw], S, invS);
  const float un = inv * xs * invS;                                  // 2^-s / S
  const float* darow = flow ? A.gates + (m + A.B) * G + 8 * hh : nullptr;
  const f16x8* w8 = reinterpret_cast<const f16x8*>(A.whht) + lane;
  float mx = 0.0f;
#pragma unroll 1
  for (int jb = 0; jb < NB; ++jb) {
    f32x16 acc = (f32x16)(0.0f);
    if (!last) {
#pragma unroll 2
      for (int ks = 0; ks < KSB; ++ks) {
        float x[8];
        pol_f4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, q1 = q0;
        if (darow) { q0 = *reinterpret_cast<const pol_f4*>(darow + 16 * ks); q1 = *reinterpret_cast<const pol_f4*>(darow + 16 * ks + 4); }
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = q0[j] * S; x[4 + j] = q1[j] * S; }
        f16x8 bf[2], a[2];
        split2(x, bf);
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) a[t2] = w8[(size_t)((t2 * NB + jb) * KSB + ks) * 64];
        acc = mfma3(a, bf, acc);
      }
    }
    if (live) {
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int u = 32 * jb + 8 * e4 + 4 * hh;
        const pol_f4 dh4 = *reinterpret_cast<const pol_f4*>(A.dh + m * H + u);
        float* g = A.gates + m * G + u;
        const pol_f4 gi = *reinterpret_cast<const pol_f4*>(g), gf = *reinterpret_cast<const pol_f4*>(g + H);
        const pol_f4 gg = *reinterpret_cast<const pol_f4*>(g + 2 * H), go = *reinterpret_cast<const pol_f4*>(g + 3 * H);
        const pol_f4 ct = *reinterpret_cast<const pol_f4*>(A.cs + m * H + u);
        pol_f4 cp = {0.0f, 0.0f, 0.0f, 0.0f}, dcn = cp;
        if (A.t == 0) cp = *reinterpret_cast<const pol_f4*>(A.c0 + b * H + u);
        else if (!fresh) cp = *reinterpret_cast<const pol_f4*>(A.cs + (m - A.B) * H + u);
        if (flow) dcn = *reinterpret_cast<const pol_f4*>(A.dcc + b * H + u);
        float tc[4];
        tanh2_f32(ct[0], ct[1], 2.8853900817779268f, tc[0], tc[1]);    // tanh(c_t) as the forward takes it
        tanh2_f32(ct[2], ct[3], 2.8853900817779268f, tc[2], tc[3]);
        pol_f4 dai, daf, dag, dao, carry;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const float th = tc[p] * down;
          const float dh = dh4[p] + acc[4 * e4 + p] * un;
          const float dc = dh * go[p] * (1.0f - th * th) + dcn[p];
          dai[p] = dc * gg[p] * (gi[p] * (1.0f - gi[p]));
          daf[p] = dc * cp[p] * (gf[p] * (1.0f - gf[p]));
          dag[p] = dc * gi[p] * (1.0f - gg[p] * gg[p]);
          dao[p] = dh * th * (go[p] * (1.0f - go[p]));
          carry[p] = dc * gf[p];
          mx = fmaxf(mx, fmaxf(fmaxf(fabsf(dai[p]), fabsf(daf[p])), fmaxf(fabsf(dag[p]), fabsf(dao[p]))));
        }
        *reinterpret_cast<pol_f4*>(g) = dai; *reinterpret_cast<pol_f4*>(g + H) = daf;
        *reinterpret_cast<pol_f4*>(g + 2 * H) = dag; *reinterpret_cast<pol_f4*>(g + 3 * H) = dao;
        *reinterpret_cast<pol_f4*>(A.dcc + b * H + u) = carry;
      }
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  if (lane == 0) A.dscale[(int64_t)A.t * nwaves + gw] = mx;
}

// ---- 4. the cell's weight gradients: a contraction over the n rows, workgroup (mt, nt, split)
struct LstmPpoWgradArgs {
  const float *da, *obs_g, *hs, *h0;   // [n, 4 H]; [T][obs_stride]; h_t [n, H]; h0_g [B, H]
  const uint8_t* start;
  float* parts;                        // [splits][part_stride]
  int64_t n, B, obs_stride;
  int32_t H, part_stride, splits;
};
// The set form: all three grid dimensions are taken, so the member is folded into z: blockIdx.z = member x max_splits + split, max_splits
// the widest member's lstm_ppo_splits.  `idle`: a split index >= the member's own lstm_ppo_splits(T B_g), or a member without columns —
// workgroup-uniform, taken before the barrier.
struct LstmPpoSetWgradArgs {
  LstmPpoSetCommon c;
  int32_t k, max_splits;
};
static_assert(sizeof(LstmPpoSetWgradArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <bool SET> using LstmPpoWgradKernelArgs = std::conditional_t<SET, LstmPpoSetWgradArgs, LstmPpoWgradArgs>;
template <bool SET>
__device__ __forceinline__ int lstm_ppo_wgrad_split(const LstmPpoWgradKernelArgs<SET>& S) {
  if constexpr (SET) return (int)blockIdx.z % S.max_splits; else return blockIdx.z;
}
template <bool SET>
__device__ __forceinline__ decltype(auto) lstm_ppo_wgrad_member(const LstmPpoWgradKernelArgs<SET>& S, bool& idle) {
  if constexpr (SET) {
    const int g = (int)blockIdx.z / S.max_splits, sp = lstm_ppo_wgrad_split<SET>(S);
    const int64_t B = S.c.table.count[g], n = S.c.T * B;
    const int splits = lstm_ppo_splits(n);
    idle = B == 0 || sp >= splits;
    LstmPpoHeadWs hd;
    LstmPpoNetWs o;
    float* ws = lstm_ppo_member_ws(S.c, g, S.k, B, hd, o);
    const LstmPpoWgradArgs M = {ws + o.gates, ws + hd.obs, ws + o.hs, ws + o.h0, reinterpret_cast<const uint8_t*>(ws + hd.start), ws + o.cparts,
                                n, B, hd.obs_stride, S.c.d.H[S.k], S.c.d.cpart[S.k], splits};
    return M;
  } else {
    idle = false;
    return (S);                                            // the arguments themselves: the plain kernel is the code it was
  }
}
template <bool SET>
__global__ __launch_bounds__(kPolBlock) void lstm_ppo_wgrad_kernel(const LstmPpoWgradKernelArgs<SET> K) {
  bool idle;
  const auto& A = lstm_ppo_wgrad_member<SET>(K, idle);
  if (SET && idle) return;
  __shared__ __attribute__((aligned(16))) float tiles[(kPolBlock / 64) * 2 * kPpoTile];   // per wave: the A tile (then its sum), the B tile
  constexpr float xs = (float)(1 << kPolXShift), inv_xs = 1.0f / xs;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int mt = blockIdx.x, nt = blockIdx.y, sp = lstm_ppo_wgrad_split<SET>(K);
  const int H = A.H, G = 4 * H;
  float* mine = tiles + wv * 2 * kPpoTile;
  _Float16* ta = reinterpret_cast<_Float16*>(mine);
  _Float16* tbt = reinterpret_cast<_Float16*>(mine + kPpoTile);
  const int64_t chunks = (A.n + 31) / 32;
  float sum[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) sum[e] = 0.0f;
  for (int64_t ch = (int64_t)sp * (kPolBlock / 64) + wv; ch < chunks; ch += (int64_t)(kPolBlock / 64) * A.splits) {
    const int64_t m = ch * 32 + r;
    const bool live = m < A.n;
    const int64_t t = live ? m / A.B : 0, b = live ? m - t * A.B : 0;
    float v[16], xb[16];
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      pol_f4 q = {0.0f, 0.0f, 0.0f, 0.0f};
      if (live) q = *reinterpret_cast<const pol_f4*>(A.da + m * G + 32 * mt + 8 * e4 + 4 * hh);
#pragma unroll
      for (int p = 0; p < 4; ++p) v[4 * e4 + p] = q[p];
    }
    float S, invS;
    wave_scale(tile_max(v), S, invS);
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] *= S;
    if (nt == 0) {
      const float* orow = A.obs_g + t * A.obs_stride + b * kPolIn;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int f = (e & 3) + 8 * (e >> 2) + 4 * hh;
        xb[e] = f < kPolIn ? (live ? lstm_ppo_operand(orow[f]) : 0.0f) : (f == kPolIn ? xs : 0.0f);   // column 17: ones (the bias gradient)
      }
    } else {
      const bool keep = live && (t == 0 || A.start[m] == 0);                                              // (1 - s_t) h_{t-1}; state0 as given
      const float* prow = keep ? (t == 0 ? A.h0 + b * H : A.hs + (m - A.B) * H) : nullptr;
      lstm_ppo_h_tile(prow, nt - 1, hh, xb);
    }
    stage_tile(ta, v, lane);
    stage_tile(tbt, xb, lane);
    wave_fence();
    f16x8 a[2][2], bf[2][2];
    load_frags(ta, lane, a);
    load_frags(tbt, lane, bf);
    f32x16 acc = (f32x16)(0.0f);
    acc = mfma3(a[0], bf[0], acc);
    acc = mfma3(a[1], bf[1], acc);
    const float unscale = invS * inv_xs;
#pragma unroll
    for (int e = 0; e < 16; ++e) sum[e] += acc[e] * unscale;
    wave_fence();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) mine[((e & 3) + 8 * (e >> 2) + 4 * hh) * 32 + r] = sum[e];
  __syncthreads();
  float* part = A.parts + (size_t)sp * A.part_stride;
  for (int el = (int)threadIdx.x; el < kPpoTile; el += kPolBlock) {
    float s = 0.0f;
    for (int k = 0; k < kPolBlock / 64; ++k) s += tiles[k * 2 * kPpoTile + el];
    const int R = 32 * mt + (el >> 5), c = el & 31;
    if (nt == 0) {
      if (c < kPolIn) part[R * kPolIn + c] = s;
      else if (c == kPolIn) part[G * kPolIn + G * H + R] = s;
    } else {
      part[G * kPolIn + R * H + 32 * (nt - 1) + c] = s;
    }
  }
}

// ---- 5. the rows of partial sums added in index order -> the gradients (divided by n; - ent_coef on d log_std) and the scalars
struct LstmPpoFinishNet {
  const float *tparts, *cparts;
  int64_t groups;
  int32_t tstride, tfloats, cstride, splits, H, grad_floats;
  float* grad;
};
struct LstmPpoFinishArgs {
  LstmPpoFinishNet net[2];
  int64_t n;
  const float* actor_block;
  float ent_coef, vf_coef;
  float* scalars;
};
__device__ __forceinline__ float lstm_ppo_finish_one(const LstmPpoFinishNet& N, int i) {
  const int G = 4 * N.H, cell = G * kPolIn + G * N.H + 2 * G;
  float sum = 0.0f;
  if (i < cell) {
    const int k = i >= cell - G ? i - G : i;                                // b_hh: the sum of b_ih
    for (int s = 0; s < N.splits; ++s) sum += N.cparts[(size_t)s * N.cstride + k];
  } else {
    for (int64_t g = 0; g < N.groups; ++g) sum += N.tparts[g * N.tstride + (i - cell)];
  }
  return sum;
}
// the set form: member blockIdx.y's rows of its piece -> row blockIdx.y of the outputs; nothing of a member without columns is written.
// `F` holds the set-wide values (the strides and sizes; grad and scalars: the outputs' row 0; the parts, groups, splits, n and
// actor_block unused).
struct LstmPpoSetFinishArgs {
  LstmPpoFinishArgs F;
  LstmPpoSetCommon c;
};
static_assert(sizeof(LstmPpoSetFinishArgs) <= 4096, "the set form's arguments fit the 4 KiB kernel-argument segment");
template <bool SET> using LstmPpoFinishKernelArgs = std::conditional_t<SET, LstmPpoSetFinishArgs, LstmPpoFinishArgs>;
template <bool SET>
__device__ __forceinline__ decltype(auto) lstm_ppo_finish_member(const LstmPpoFinishKernelArgs<SET>& S, bool& idle) {
  if constexpr (SET) {
    const int g = blockIdx.y;
    const int64_t B = S.c.table.count[g], n = S.c.T * B;
    idle = B == 0;
    LstmPpoHeadWs hd;
    LstmPpoNetWs oa, oc;
    float* ws = lstm_ppo_member_ws(S.c, g, 0, B, hd, oa);
    lstm_ppo_member_ws(S.c, g, 1, B, hd, oc);
    LstmPpoFinishArgs F = S.F;
    F.n = n;
    F.net[0].tparts = ws + oa.tparts; F.net[0].cparts = ws + oa.cparts;
    F.net[1].tparts = ws + oc.tparts; F.net[1].cparts = ws + oc.cparts;
    F.net[0].groups = F.net[1].groups = lstm_ppo_trunk_groups(n);
    F.net[0].splits = F.net[1].splits = lstm_ppo_splits(n);
    F.net[0].grad = S.F.net[0].grad + (size_t)g * S.F.net[0].grad_floats;
    F.net[1].grad = S.F.net[1].grad + (size_t)g * S.F.net[1].grad_floats;
    F.actor_block = lstm_ppo_member_block(S.c, g, 0);
    F.scalars = S.F.scalars + (size_t)g * kPpoScalars;
    return F;
  } else {
    idle = false;
    return (S);                                            // the arguments themselves: the plain kernel is the code it was
  }
}
template <bool SET>
__global__ __launch_bounds__(256) void lstm_ppo_finish_kernel(const LstmPpoFinishKernelArgs<SET> S) {
  bool idle;
  const auto& F = lstm_ppo_finish_member<SET>(S, idle);
  if (SET && idle) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float fn = (float)F.n;
  const int Ga = F.net[0].grad_floats, Gc = F.net[1].grad_floats;
  if (i < Ga) {
    float v = lstm_ppo_finish_one(F.net[0], i) / fn;
    if (i >= Ga - kPolOut) v -= F.ent_coef;
    F.net[0].grad[i] = v;
  } else if (i < Ga + Gc) {
    F.net[1].grad[i - Ga] = lstm_ppo_finish_one(F.net[1], i - Ga) / fn;
  } else if (i == Ga + Gc) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const LstmPpoFinishNet &a = F.net[0], &c = F.net[1];
    for (int64_t g = 0; g < a.groups; ++g)
      for (int k = 0; k < 3; ++k) s[k] += (double)a.tparts[g * a.tstride + a.tstride - 4 + k];
    for (int64_t g = 0; g < c.groups; ++g) s[3] += (double)c.tparts[g * c.tstride + c.tstride - 1];
    ppo_finish_scalars(s, F.n, F.actor_block + kMlpStd + 8, F.ent_coef, F.vf_coef, F.scalars);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr int kLstmPpoTrunkLds = (kPolBlock / 64) * (kPpoWaveTiles + 4) * 4;   // 98,432 B

// c != c_out, h != h_next: a step reads step t - 1's rows and writes step t's
static void lstm_launch_cell_keep(int H, const float* W, const float* obs, const uint8_t* start, const float* h, const float* c, float* h_next, float* c_out,
                           float* gates, int64_t n, hipStream_t s) {
  switch (H) {
    case 32: hipLaunchKernelGGL(lstm_cell_keep_kernel<32>, dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, gates, n); break;
    case 64: hipLaunchKernelGGL(lstm_cell_keep_kernel<64>, dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, gates, n); break;
    case 128: hipLaunchKernelGGL(lstm_cell_keep_kernel<128>, dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, gates, n); break;
    default: hipLaunchKernelGGL(lstm_cell_keep_kernel<256>, dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, gates, n); break;
  }
}

static void lstm_launch_cell_keep_set(int H, const LstmPpoSetCellArgs& A, dim3 grid, hipStream_t s) {
  switch (H) {
    case 32: hipLaunchKernelGGL(lstm_cell_keep_set_kernel<32>, grid, dim3(kPolBlock), 0, s, A); break;
    case 64: hipLaunchKernelGGL(lstm_cell_keep_set_kernel<64>, grid, dim3(kPolBlock), 0, s, A); break;
    case 128: hipLaunchKernelGGL(lstm_cell_keep_set_kernel<128>, grid, dim3(kPolBlock), 0, s, A); break;
    default: hipLaunchKernelGGL(lstm_cell_keep_set_kernel<256>, grid, dim3(kPolBlock), 0, s, A); break;
  }
}

template <bool ACTOR, bool SET>
static const void* trunk_kernel_of(int activation) {
  switch (activation) {
    case RDV_ACT_RELU: return reinterpret_cast<const void*>(lstm_ppo_trunk_kernel<RDV_ACT_RELU, ACTOR, SET>);
    case RDV_ACT_SIGMOID: return reinterpret_cast<const void*>(lstm_ppo_trunk_kernel<RDV_ACT_SIGMOID, ACTOR, SET>);
    default: return reinterpret_cast<const void*>(lstm_ppo_trunk_kernel<RDV_ACT_TANH, ACTOR, SET>);
  }
}
hipError_t lstm_ppo_raise_lds_limit() {
  for (int act = 0; act < 3; ++act)
    for (const void* k : {trunk_kernel_of<true, false>(act), trunk_kernel_of<false, false>(act), trunk_kernel_of<true, true>(act), trunk_kernel_of<false, true>(act)}) {
      hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLstmPpoTrunkLds);
      if (err != hipSuccess) return err;
    }
  return hipSuccess;
}
template <bool ACTOR, bool SET>
static void launch_trunk(int activation, const LstmPpoTrunkKernelArgs<SET>& A, dim3 grid, hipStream_t s) {
  switch (activation) {
    case RDV_ACT_RELU: hipLaunchKernelGGL((lstm_ppo_trunk_kernel<RDV_ACT_RELU, ACTOR, SET>), grid, dim3(kPolBlock), kLstmPpoTrunkLds, s, A); break;
    case RDV_ACT_SIGMOID: hipLaunchKernelGGL((lstm_ppo_trunk_kernel<RDV_ACT_SIGMOID, ACTOR, SET>), grid, dim3(kPolBlock), kLstmPpoTrunkLds, s, A); break;
    default: hipLaunchKernelGGL((lstm_ppo_trunk_kernel<RDV_ACT_TANH, ACTOR, SET>), grid, dim3(kPolBlock), kLstmPpoTrunkLds, s, A); break;
  }
}
template <bool SET>
static void launch_bptt(int H, const LstmPpoBpttKernelArgs<SET>& A, dim3 grid, hipStream_t s) {
  switch (H) {
    case 32: hipLaunchKernelGGL((lstm_ppo_bptt_kernel<32, SET>), grid, dim3(kPolBlock), 0, s, A); break;
    case 64: hipLaunchKernelGGL((lstm_ppo_bptt_kernel<64, SET>), grid, dim3(kPolBlock), 0, s, A); break;
    case 128: hipLaunchKernelGGL((lstm_ppo_bptt_kernel<128, SET>), grid, dim3(kPolBlock), 0, s, A); break;
    default: hipLaunchKernelGGL((lstm_ppo_bptt_kernel<256, SET>), grid, dim3(kPolBlock), 0, s, A); break;
  }
}
// the workgroups of lstm_ppo_transpose_kernel: the fragments of the net that has more
static unsigned lstm_ppo_transpose_frags(const LstmPpoNet& a, const LstmPpoNet& c) {
  int frags = 0;
  for (const LstmPpoNet* N : {&a, &c}) {
    const int f = (N->whht_floats + N->w0t_floats) / (kPolFragBytes / 4);
    if (f > frags) frags = f;
  }
  return (unsigned)frags;
}
// the x-workgroups of lstm_ppo_gather_kernel for B columns of T steps
static unsigned lstm_ppo_gather_groups(int64_t T, int64_t B) {
  const int64_t n = T * B, most = n * kPolIn > B * kLstmMaxH ? n * kPolIn : B * kLstmMaxH;
  return (unsigned)((most + 255) / 256);
}

void lstm_ppo_launch(const LstmPpoLaunch& a, hipStream_t s) {
  const int64_t T = a.n_steps, B = a.n_seq, n = T * B;
  LstmPpoWs W;
  lstm_ppo_workspace(a.actor, a.critic, T, B, W);
  float* ws = a.workspace;
  uint8_t* start_g = reinterpret_cast<uint8_t*>(ws + W.start);
  const LstmPpoNet* nets[2] = {&a.actor, &a.critic};
  const float* blocks[2] = {a.actor_block, a.critic_block};
  const int acts[2] = {a.actor_act, a.critic_act};
  const int splits = lstm_ppo_splits(n);

  // 0. the gathered columns and the transposed fragments
  {
    LstmPpoGatherArgs g = {a.obs, a.done, {a.actor_h0, a.actor_c0, a.critic_h0, a.critic_c0}, a.envs, ws + W.obs, start_g,
                           {ws + W.net[0].h0, ws + W.net[0].c0, ws + W.net[1].h0, ws + W.net[1].c0}, a.n_envs, B, T, W.obs_stride, a.actor.H, a.critic.H};
    hipLaunchKernelGGL(lstm_ppo_gather_kernel<false>, dim3(lstm_ppo_gather_groups(T, B), 6), dim3(256), 0, s, g);
    ppo_mlp_launch_transpose(a.actor_block, a.critic_block, ws, s);
    LstmPpoTransposeArgs tr = {{a.actor_block, a.critic_block}, {ws + W.net[0].whht, ws + W.net[1].whht}, {ws + W.net[0].w0t, ws + W.net[1].w0t}};
    hipLaunchKernelGGL(lstm_ppo_transpose_kernel<false>, dim3(lstm_ppo_transpose_frags(a.actor, a.critic), 2), dim3(512), 0, s, tr);
  }
  const PpoRowArgs rows = {a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, nullptr, n, a.k.clip_lo, a.k.clip_hi, a.k.clip_range, 2.0f * a.k.vf_coef};
  for (int k = 0; k < 2; ++k) {
    const LstmPpoNet& N = *nets[k];
    const LstmPpoNetWs& o = W.net[k];
    const int H = N.H;
    // 1. the forward replay
    for (int64_t t = 0; t < T; ++t) {
      const float* h_in = t == 0 ? ws + o.h0 : ws + o.hs + (t - 1) * B * H;
      const float* c_in = t == 0 ? ws + o.c0 : ws + o.cs + (t - 1) * B * H;
      lstm_launch_cell_keep(H, blocks[k], ws + W.obs + t * W.obs_stride, t == 0 ? nullptr : start_g + t * B, h_in, c_in, ws + o.hs + t * B * H,
                            ws + o.cs + t * B * H, ws + o.gates + t * B * 4 * H, B, s);
    }
    // 2. the trunk
    const int64_t groups = ppo_mlp_workgroups(N.T, n);
    LstmPpoTrunkArgs tr = {blocks[k], ws + (size_t)k * kPpoMlpBwdFloats, ws + o.w0t, ws + o.hs, rows, a.envs, a.n_envs, B, ws + o.tparts,
                           k == 0 ? a.log_prob : a.values, ws + o.dh, H, N.T};
    if (k == 0) launch_trunk<true, false>(acts[k], tr, dim3((unsigned)groups), s);
    else launch_trunk<false, false>(acts[k], tr, dim3((unsigned)groups), s);
    // 3. back through time
    for (int64_t t = T - 1; t >= 0; --t) {
      LstmPpoBpttArgs bp = {blocks[k], ws + o.whht, ws + o.cs, ws + o.c0, ws + o.dh, ws + o.gates, ws + o.dcc, ws + o.dscale, start_g, B, (int32_t)T, (int32_t)t};
      launch_bptt<false>(H, bp, dim3((unsigned)((B + kPolBlockEnvs - 1) / kPolBlockEnvs)), s);
    }
    // 4. the cell's weight gradients
    LstmPpoWgradArgs wg = {ws + o.gates, ws + W.obs, ws + o.hs, ws + o.h0, start_g, ws + o.cparts, n, B, W.obs_stride, H, (int32_t)lstm_ppo_up4(N.cell_part), splits};
    hipLaunchKernelGGL(lstm_ppo_wgrad_kernel<false>, dim3((unsigned)(4 * H / 32), (unsigned)(1 + H / 32), (unsigned)splits), dim3(kPolBlock), 0, s, wg);
  }
  // 5. the sums
  LstmPpoFinishArgs F;
  float* grads[2] = {a.actor_grad, a.critic_grad};
  for (int k = 0; k < 2; ++k) {
    const LstmPpoNet& N = *nets[k];
    F.net[k] = {ws + W.net[k].tparts, ws + W.net[k].cparts, ppo_mlp_workgroups(N.T, n), N.T.part_floats, N.T.grad_floats, (int32_t)lstm_ppo_up4(N.cell_part),
                splits, N.H, N.grad_floats, grads[k]};
  }
  F.n = n; F.actor_block = a.actor_block; F.ent_coef = a.k.ent_coef; F.vf_coef = a.k.vf_coef; F.scalars = a.scalars;
  const int total = a.actor.grad_floats + a.critic.grad_floats + 1;
  hipLaunchKernelGGL(lstm_ppo_finish_kernel<false>, dim3((total + 255) / 256), dim3(256), 0, s, F);
}

// The set form: the launches of lstm_ppo_launch, 4 T + 8 whatever the member count, each over the widest member's grid times the members.
void lstm_ppo_set_launch(const LstmPpoSetLaunch& L, hipStream_t s) {
  const LstmPpoLaunch& a = L.a;
  const unsigned P = (unsigned)L.n_members;
  const int64_t T = a.n_steps, Bmax = L.max_count, nmax = T * Bmax;
  const int acts[2] = {a.actor_act, a.critic_act};
  const LstmPpoNet* nets[2] = {&a.actor, &a.critic};
  const int max_splits = lstm_ppo_splits(nmax);
  const LstmPpoSetCommon c = {{a.actor_block, a.critic_block}, {L.actor_block_floats, L.critic_block_floats}, a.workspace, T, lstm_ppo_dims(a.actor, a.critic), L.table};

  // 0. the gathered columns and the transposed fragments
  {
    LstmPpoSetGatherArgs g = {{a.obs, a.done, {a.actor_h0, a.actor_c0, a.critic_h0, a.critic_c0}, a.envs, nullptr, nullptr, {nullptr, nullptr, nullptr, nullptr},
                               a.n_envs, 0, T, 0, a.actor.H, a.critic.H}, c};
    hipLaunchKernelGGL(lstm_ppo_gather_kernel<true>, dim3(lstm_ppo_gather_groups(T, Bmax), 6, P), dim3(256), 0, s, g);
    ppo_mlp_launch_set_transpose(a.actor_block, a.critic_block, a.workspace, L.actor_block_floats, L.critic_block_floats, L.n_members, L.table, s);
    hipLaunchKernelGGL(lstm_ppo_transpose_kernel<true>, dim3(lstm_ppo_transpose_frags(a.actor, a.critic), 2, P), dim3(512), 0, s, c);
  }
  const PpoRowArgs rows = {a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, nullptr, 0, a.k.clip_lo, a.k.clip_hi, a.k.clip_range, 2.0f * a.k.vf_coef};
  const dim3 columns((unsigned)((Bmax + kPolBlockEnvs - 1) / kPolBlockEnvs), P);
  for (int k = 0; k < 2; ++k) {
    const LstmPpoNet& N = *nets[k];
    const int H = N.H;
    // 1. the forward replay
    for (int64_t t = 0; t < T; ++t) lstm_launch_cell_keep_set(H, {c, k, (int32_t)t}, columns, s);
    // 2. the trunk
    LstmPpoSetTrunkArgs tr = {{nullptr, nullptr, nullptr, nullptr, rows, a.envs, a.n_envs, 0, nullptr, k == 0 ? a.log_prob : a.values, nullptr, H, N.T}, c};
    const dim3 groups((unsigned)lstm_ppo_trunk_groups(nmax), P);
    if (k == 0) launch_trunk<true, true>(acts[k], tr, groups, s);
    else launch_trunk<false, true>(acts[k], tr, groups, s);
    // 3. back through time
    for (int64_t t = T - 1; t >= 0; --t) launch_bptt<true>(H, {c, k, (int32_t)t}, columns, s);
    // 4. the cell's weight gradients
    LstmPpoSetWgradArgs wg = {c, k, max_splits};
    hipLaunchKernelGGL(lstm_ppo_wgrad_kernel<true>, dim3((unsigned)(4 * H / 32), (unsigned)(1 + H / 32), (unsigned)max_splits * P), dim3(kPolBlock), 0, s, wg);
  }
  // 5. the sums
  LstmPpoSetFinishArgs F;
  float* grads[2] = {a.actor_grad, a.critic_grad};
  for (int k = 0; k < 2; ++k) {
    const LstmPpoNet& N = *nets[k];
    F.F.net[k] = {nullptr, nullptr, 0, N.T.part_floats, N.T.grad_floats, (int32_t)lstm_ppo_up4(N.cell_part), 0, N.H, N.grad_floats, grads[k]};
  }
  F.F.n = 0; F.F.actor_block = nullptr; F.F.ent_coef = a.k.ent_coef; F.F.vf_coef = a.k.vf_coef; F.F.scalars = a.scalars;
  F.c = c;
  const int total = a.actor.grad_floats + a.critic.grad_floats + 1;
  hipLaunchKernelGGL(lstm_ppo_finish_kernel<true>, dim3((total + 255) / 256, P), dim3(256), 0, s, F);
}

}  // namespace rdv

// rdv_ppo_lstm_adam.hip — the kernels of rdv_ppo_lstm_adam.h and their launch, in a translation unit of its own (the objects of the other
// units do not change when it does).  The exported rdv_lstm_ppo_set_adam_step is in rdv_policy_host.hip, with the other policy entry points.
//
// The elementwise contract of include/rdv.h is float32 with every operation rounded on its own: nothing in this unit may be contracted
// into an fma.  `/` and sqrtf are hipcc's correctly rounded ones (its default; the v_fma of their expansions are theirs).
#pragma clang fp contract(off)
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_policy_mlp.h"
#include "rdv_ppo_lstm_adam.h"

namespace rdv {

static_assert(kLstmAdamPerThread * kPpoAdamThreads == kLstmAdamChunk, "a chunk is a whole number of entries per thread");

__device__ __forceinline__ bool lstm_adam_active(const PpoAdamLaunch& a, int g) { return (a.mask >> g) & 1; }
__device__ __forceinline__ double* lstm_adam_sums(const LstmAdamLaunch& A, int g) {
  return reinterpret_cast<double*>(A.ws + (size_t)g * (size_t)A.member_bytes);
}
// the partial maxima of (net, packer layer): one float per chunk
__device__ __forceinline__ float* lstm_adam_maxima(const LstmAdamLaunch& A, int g, int net, int layer) {
  return reinterpret_cast<float*>(A.ws + (size_t)g * (size_t)A.member_bytes + A.maxima_at) + (size_t)(net * kLstmAdamPackLayers + layer) * A.chunks;
}
// packer layer l of a net: the entries [lo, hi) of its row whose max |w| sets the layer's shift
__device__ __forceinline__ void lstm_adam_layer_range(const LstmAdamNet& N, int l, int& lo, int& hi) {
  if (l == 0) { lo = 0; hi = N.cell_w; return; }
  lo = N.cell_floats + N.T.w_off[l - 1];
  hi = lo + N.T.out_w[l - 1] * N.T.in_w[l - 1];
}

// ---- 1. the sums of squares of the chunks of [actor row | critic row]
__global__ __launch_bounds__(kPpoAdamThreads) void lstm_adam_sumsq_kernel(const LstmAdamLaunch A) {
  const PpoAdamLaunch& a = A.a;
  const int c = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  if (!lstm_adam_active(a, g)) return;                             // (workgroup-uniform) an inactive member: nothing read, nothing written
  __shared__ double part[kPpoAdamThreads];
  const int na = a.ga, nc = a.gc;
  const float* ga = a.actor_grad + (size_t)g * na;
  const float* gc = a.critic_grad + (size_t)g * nc;
  const int lo = c * kLstmAdamChunk, hi = min(lo + kLstmAdamChunk, na + nc);
  double s = 0.0;
  for (int i = lo + t; i < hi; i += kPpoAdamThreads) {
    const double x = (double)(i < na ? ga[i] : gc[i - na]);
    s += x * x;                                                    // (the product of two floats is exact in double)
  }
  part[t] = s;
  for (int w = kPpoAdamThreads / 2; w > 0; w >>= 1) {              // a fixed tree: the order depends on the index alone
    __syncthreads();
    if (t < w) part[t] += part[t + w];
  }
  if (t == 0) lstm_adam_sums(A, g)[c] = part[0];
}

// ---- 2. the chunk sums in index order, then the member's coefficients
__global__ __launch_bounds__(64) void lstm_adam_coef_kernel(const LstmAdamLaunch A) {
  const int g = blockIdx.x;
  if (!lstm_adam_active(A.a, g) || threadIdx.x != 0) return;
  const double* sums = lstm_adam_sums(A, g);
  double s = 0.0;
  for (int c = 0; c < A.sum_chunks; ++c) s += sums[c];
  adam_member_coef(A.a, g, s);
}

// ---- 3. the elementwise step of one chunk of one net's row, and the chunk's max |p_new| per packer layer
__global__ __launch_bounds__(kPpoAdamThreads) void lstm_adam_step_kernel(const LstmAdamLaunch A) {
  const PpoAdamLaunch& a = A.a;
  const int c = blockIdx.x, net = blockIdx.y, g = blockIdx.z, t = threadIdx.x;
  if (!lstm_adam_active(a, g)) return;                             // (the three tests are workgroup-uniform and ahead of every barrier)
  const LstmAdamNet& N = A.net[net];
  if (c >= N.chunks) return;                                       // the shorter net
  const float4 k = *reinterpret_cast<const float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (a.coef[(size_t)g * kPpoAdamCoef + 4] != 0.0f) return;        // a non-finite norm: the member is skipped whole
  const float clip = k.y, step_size = k.z, isb2 = k.w;
  const bool actor = net == 0;
  const int count = N.grad_floats, packed = N.T.L + 2;
  const size_t row = (size_t)g * (size_t)count;
  const float* gr = (actor ? a.actor_grad : a.critic_grad) + row;
  float* p = (actor ? a.actor_param : a.critic_param) + row;
  float* m = (actor ? a.actor_m : a.critic_m) + row;
  float* v = (actor ? a.actor_v : a.critic_v) + row;

  const int base = c * kLstmAdamChunk + t;
  float pn[kLstmAdamPerThread];
#pragma unroll
  for (int j = 0; j < kLstmAdamPerThread; ++j) {
    const int i = base + j * kPpoAdamThreads;
    pn[j] = i < count ? adam_element(a, gr, m, v, p, i, clip, step_size, isb2) : 0.0f;
  }

  // max |w| per packer layer: the thread's, the wave's, the workgroup's (a maximum does not depend on the order)
  __shared__ float red[(kPpoAdamThreads / 64) * kLstmAdamPackLayers];
  for (int l = 0; l < packed; ++l) {
    int lo, hi;
    lstm_adam_layer_range(N, l, lo, hi);
    float mx = 0.0f;
#pragma unroll
    for (int j = 0; j < kLstmAdamPerThread; ++j) {
      const int i = base + j * kPpoAdamThreads;
      if (i >= lo && i < hi) mx = fmaxf(mx, fabsf(pn[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[(t >> 6) * kLstmAdamPackLayers + l] = mx;
  }
  __syncthreads();
  if (t < packed) {
    float all = red[t];
#pragma unroll
    for (int wv = 1; wv < kPpoAdamThreads / 64; ++wv) all = fmaxf(all, red[wv * kLstmAdamPackLayers + t]);
    lstm_adam_maxima(A, g, net, t)[c] = all;
  }
}

// ---- 4. the repack of one net's forward block [trunk block | cell block] from its master row
__global__ __launch_bounds__(kPpoAdamThreads) void lstm_adam_pack_kernel(const LstmAdamLaunch A) {
  const PpoAdamLaunch& a = A.a;
  const int net = blockIdx.y, g = blockIdx.z, t = threadIdx.x;
  if (!lstm_adam_active(a, g)) return;                             // (the three tests are workgroup-uniform and ahead of every barrier)
  const LstmAdamNet& N = A.net[net];
  if ((int)blockIdx.x * kPpoAdamThreads >= N.items) return;
  if (a.coef[(size_t)g * kPpoAdamCoef + 4] != 0.0f) return;        // a non-finite norm: the member is skipped whole
  const bool actor = net == 0;
  const int L = N.T.L, packed = L + 2, H = N.H;

  // the shifts: shs[0] the cell's, shs[1 + l] the trunk's layer l
  __shared__ float red[(kPpoAdamThreads / 64) * kLstmAdamPackLayers];
  __shared__ int shs[kLstmAdamPackLayers];
  for (int l = 0; l < packed; ++l) {
    const float* part = lstm_adam_maxima(A, g, net, l);
    float mx = 0.0f;
    for (int c = t; c < N.chunks; c += kPpoAdamThreads) mx = fmaxf(mx, part[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[(t >> 6) * kLstmAdamPackLayers + l] = mx;
  }
  __syncthreads();
  if (t < packed) {
    float all = red[t];
#pragma unroll
    for (int wv = 1; wv < kPpoAdamThreads / 64; ++wv) all = fmaxf(all, red[wv * kLstmAdamPackLayers + t]);
    shs[t] = adam_shift(all);
  }
  __syncthreads();

  const float* p = (actor ? a.actor_param : a.critic_param) + (size_t)g * (size_t)N.grad_floats;
  float* block = (actor ? a.actor_block : a.critic_block) + (size_t)g * (size_t)N.block_floats;
  float* cell = block + N.cell_at;
  const int q = (int)blockIdx.x * kPpoAdamThreads + t;
  const int lane = q & 63, r = lane & 31, h = lane >> 5;
  if (q < N.frags_trunk * 64) {
    // a trunk fragment: fragment (term MT + mt) KS + ks of layer l's 2 MT KS; one 16-byte store per (fragment, lane)
    const int f = q >> 6;
    int l = 0;
    while (f >= N.frag0[l + 1]) ++l;
    const int fl = f - N.frag0[l], MT = N.T.mt[l], KS = N.T.ks[l], in_w = N.T.in_w[l], out_w = N.T.out_w[l], sft = shs[1 + l];
    const int term = fl / (MT * KS), mt = (fl / KS) % MT, ks = fl % KS;
    const int orow = 32 * mt + r;
    const float* w = p + N.cell_floats + N.T.w_off[l];
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kk = l == 0 ? adam_k_natural(ks, h, j) : adam_k_accumulator(ks, h, j);
      const float x = (orow < out_w && kk < in_w) ? w[orow * in_w + kk] : 0.0f;
      o[j] = adam_split_term(x, sft, term);
    }
    *reinterpret_cast<f16x8*>(block + kMlpHdr + 4 * (size_t)q) = o;
    return;
  }
  if (q < N.frags_all * 64) {
    // a cell fragment: [W_ih | W_hh] as one matrix of 4 H rows over 32 (17 used) + H columns, natural k order, one shift
    const int qc = q - N.frags_trunk * 64, f = qc >> 6, TL = N.cell_tiles, KS = N.cell_ks, NB = H / 32, sft = shs[0];
    const int term = f / (TL * KS), tile = (f / KS) % TL, ks = f % KS;
    const int row = (tile / NB) * H + 32 * (tile % NB) + r;         // gate tile / NB, units 32 (tile % NB) .. of it
    const float* w_ih = p + row * kPolIn;
    const float* w_hh = p + 4 * H * kPolIn + (size_t)row * H;
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kk = adam_k_natural(ks < 2 ? ks : ks - 2, h, j);
      const float x = ks < 2 ? (kk < kPolIn ? w_ih[kk] : 0.0f) : w_hh[kk];
      o[j] = adam_split_term(x, sft, term);
    }
    *reinterpret_cast<f16x8*>(cell + kLstmCellHdr + 4 * (size_t)qc) = o;
    return;
  }
  int e = q - N.frags_all * 64;
  if (e < N.tiles_trunk * 32) {
    // a trunk bias: [mt][h][16] per layer behind the fragments, times the accumulator's scale; padded rows zero
    const int tile = e >> 5;
    int l = 0;
    while (tile >= N.tile0[l + 1]) ++l;
    const int orow = adam_bias_row(e - 32 * N.tile0[l]);
    block[kMlpHdr + N.frags_trunk * (kPolFragBytes / 4) + e] =
        orow < N.T.out_w[l] ? p[N.cell_floats + N.T.b_off[l] + orow] * ldexpf(1.0f, kPolXShift + shs[1 + l]) : 0.0f;
    return;
  }
  e -= N.tiles_trunk * 32;
  if (e < 2 * N.cell_tiles * 32) {
    // a cell bias: b_ih, then b_hh, each [tile][h][16] in accumulator order, times the accumulator's scale
    const int which = e / (N.cell_tiles * 32), tl = e % (N.cell_tiles * 32), tile = tl >> 5, NB = H / 32;
    const int row = (tile / NB) * H + 32 * (tile % NB) + adam_bias_row(tl & 31);
    cell[kLstmCellHdr + (size_t)2 * N.cell_tiles * N.cell_ks * (kPolFragBytes / 4) + e] = p[N.cell_w + which * 4 * H + row] * ldexpf(1.0f, kPolXShift + shs[0]);
    return;
  }
  e -= 2 * N.cell_tiles * 32;
  // each layer's inverse accumulator scale (a power of two: exact); an actor's exp(log_std) and log_std
  if (e <= L) { block[kMlpRec + kMlpRecStride * e + 4] = ldexpf(1.0f, -(kPolXShift + shs[1 + e])); return; }
  if (e == L + 1) { cell[0] = ldexpf(1.0f, -(kPolXShift + shs[0])); return; }
  e -= L + 2;
  if (actor && e < kPolOut) {
    const float ls = p[N.cell_floats + N.T.ls_off + e];
    block[kMlpStd + e] = (float)exp((double)ls);
    block[kMlpStd + 8 + e] = ls;
  }
}

void lstm_adam_launch(const LstmAdamLaunch& L, hipStream_t s) {
  const unsigned P = (unsigned)L.a.n_members;
  const int items = L.net[0].items > L.net[1].items ? L.net[0].items : L.net[1].items;
  hipLaunchKernelGGL(lstm_adam_sumsq_kernel, dim3((unsigned)L.sum_chunks, P), dim3(kPpoAdamThreads), 0, s, L);
  hipLaunchKernelGGL(lstm_adam_coef_kernel, dim3(P), dim3(64), 0, s, L);
  hipLaunchKernelGGL(lstm_adam_step_kernel, dim3((unsigned)L.chunks, 2, P), dim3(kPpoAdamThreads), 0, s, L);
  hipLaunchKernelGGL(lstm_adam_pack_kernel, dim3((unsigned)((items + kPpoAdamThreads - 1) / kPpoAdamThreads), 2, P), dim3(kPpoAdamThreads), 0, s, L);
}

}  // namespace rdv

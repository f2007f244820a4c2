// rdv_ppo_adam.hip — the kernels of rdv_ppo_adam.h and their launch, in a translation unit of its own (the objects of the other units do
// not change when it does).  The exported rdv_ppo_set_adam_step is in rdv_policy_host.hip, with the other policy entry points.
//
// The elementwise contract of include/rdv.h is float32 with every operation rounded on its own: nothing in this unit may be contracted
// into an fma.  `/` and sqrtf are hipcc's correctly rounded ones (its default; the v_fma of their expansions are theirs).
#pragma clang fp contract(off)
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_policy_mlp.h"
#include "rdv_ppo_adam.h"

namespace rdv {

constexpr int kAdamAll = kPpoActorGrad + kPpoCriticGrad;          // 11,085 entries under one norm
constexpr int kAdamLogStd = kPpoW3 + kPolOut * kPolHid + kPolOut;   // 5702: log_std inside the actor's flat vector
static_assert(kAdamLogStd + kPolOut == kPpoActorGrad && kPpoW3 + kPolHid + 1 == kPpoCriticGrad, "the flat layouts of RdvPpoOut");
static_assert(kPolF32 == 32 * 64 * 4 && kPolFloats - kPolF32 == 180 && kPolB1 == kPolF32 && kPolB3 == kPolF32 + 128 && kPolStd == kPolF32 + 160 &&
              kPolLogStd == kPolF32 + 168 && kPolScale == kPolF32 + 176, "the fp32 section as ppo_adam_tail lays it out");

// ---- 1. one norm, one clip coefficient and the two step coefficients per member
__global__ __launch_bounds__(kPpoAdamThreads) void ppo_adam_norm_kernel(const PpoAdamLaunch a) {
  const int g = blockIdx.x, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (workgroup-uniform) an inactive member: nothing read, nothing written
  __shared__ double part[kPpoAdamThreads];
  const float* ga = a.actor_grad + (size_t)g * kPpoActorGrad;
  const float* gc = a.critic_grad + (size_t)g * kPpoCriticGrad;
  double s = 0.0;
  for (int i = t; i < kAdamAll; i += kPpoAdamThreads) {
    const double x = (double)(i < kPpoActorGrad ? ga[i] : gc[i - kPpoActorGrad]);
    s += x * x;                                                    // (the product of two floats is exact in double)
  }
  part[t] = s;
  for (int w = kPpoAdamThreads / 2; w > 0; w >>= 1) {              // a fixed tree: the order depends on the index alone
    __syncthreads();
    if (t < w) part[t] += part[t + w];
  }
  if (t != 0) return;
  const float total = (float)sqrt(part[0]);
  float4* c = reinterpret_cast<float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (!(fabsf(total) <= 3.402823466e+38f)) {                       // inf or NaN: the member is skipped whole
    c[0] = make_float4(total, 0.0f, 0.0f, 0.0f);
    c[1] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  // PyTorch's expression on the stored float norm, taken in double and rounded to float once, as the two step coefficients are
  const float clip = (float)fmin(1.0, (double)a.max_grad_norm / ((double)total + (double)1e-6f));
  const int64_t tt = a.step[g] + 1;
  const double bc1 = 1.0 - pow(a.beta1, (double)tt), bc2 = 1.0 - pow(a.beta2, (double)tt);
  c[0] = make_float4(total, clip, (float)(a.lr / bc1), (float)(1.0 / sqrt(bc2)));
  c[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  a.step[g] = tt;
}

// pol_layer_shift's rule on the layer's max |w|
__device__ __forceinline__ int adam_shift(float mx) {
  int sft = 10;
  while (sft > -20 && ldexpf(mx, sft) >= 32768.0f) --sft;
  return sft;
}

// float f (0 .. 179) of the block's fp32 section, from the net's new parameters `w` (LDS, the flat layout)
__device__ __forceinline__ float ppo_adam_tail(const float* w, int f, bool actor, int out_dim, int sh1, int sh2, int sh3) {
  if (f < 160) {                                                   // the biases in accumulator order, times the accumulator's scale
    const int layer = f >> 6, i = f & 63, mt = i >> 5, h = (i >> 4) & 1, e = i & 15;
    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
    if (layer == 2) return (mt == 0 && row < out_dim) ? w[kPpoW3 + out_dim * kPolHid + row] * ldexpf(1.0f, kPolXShift + sh3) : 0.0f;
    return w[(layer ? kPpoB2 : kPpoB1) + 32 * mt + row] * ldexpf(1.0f, kPolXShift + (layer ? sh2 : sh1));
  }
  if (f < 176) {                                                   // exp(log_std) [8], log_std [8]; a critic's are zero
    const int j = (f - 160) & 7;
    if (!actor || j >= kPolOut) return 0.0f;
    const float ls = w[kAdamLogStd + j];
    return f < 168 ? (float)exp((double)ls) : ls;
  }
  const int l = f - 176;                                           // the inverse scales (powers of two: exact), one zero
  return l == 3 ? 0.0f : ldexpf(1.0f, -(kPolXShift + (l == 0 ? sh1 : l == 1 ? sh2 : sh3)));
}

// ---- 2. the step and the repack of one member's net
__global__ __launch_bounds__(kPpoAdamThreads) void ppo_adam_update_kernel(const PpoAdamLaunch a) {
  const int net = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (both tests are workgroup-uniform and ahead of every barrier)
  const float4 c = *reinterpret_cast<const float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (a.coef[(size_t)g * kPpoAdamCoef + 4] != 0.0f) return;        // a non-finite norm: the member is skipped whole
  const float clip = c.y, step_size = c.z, isb2 = c.w;

  __shared__ __attribute__((aligned(16))) float w[kPpoActorGrad];
  __shared__ float red[(kPpoAdamThreads / 64) * 3];
  const bool actor = net == 0;
  const int count = actor ? kPpoActorGrad : kPpoCriticGrad, out_dim = actor ? kPolOut : 1;
  const size_t row = (size_t)g * (size_t)count;
  const float* gr = (actor ? a.actor_grad : a.critic_grad) + row;
  float* p = (actor ? a.actor_param : a.critic_param) + row;
  float* m = (actor ? a.actor_m : a.critic_m) + row;
  float* v = (actor ? a.actor_v : a.critic_v) + row;

  for (int i = t; i < count; i += kPpoAdamThreads) {
    const float gp = gr[i] * clip;
    const float mo = m[i];
    const float mn = mo + (gp - mo) * a.omb1;
    const float vn = v[i] * a.b2 + (a.omb2 * gp) * gp;
    const float pn = p[i] - step_size * (mn / (sqrtf(vn) * isb2 + a.eps));
    m[i] = mn; v[i] = vn; p[i] = pn;
    w[i] = pn;
  }
  __syncthreads();

  // max |w| per layer: the thread's, the wave's, the workgroup's (a maximum does not depend on the order)
  float mx[3] = {0.0f, 0.0f, 0.0f};
  for (int i = t; i < kPolHid * kPolIn; i += kPpoAdamThreads) mx[0] = fmaxf(mx[0], fabsf(w[kPpoW1 + i]));
  for (int i = t; i < kPolHid * kPolHid; i += kPpoAdamThreads) mx[1] = fmaxf(mx[1], fabsf(w[kPpoW2 + i]));
  for (int i = t; i < out_dim * kPolHid; i += kPpoAdamThreads) mx[2] = fmaxf(mx[2], fabsf(w[kPpoW3 + i]));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
    if ((t & 63) == 0) red[(t >> 6) * 3 + k] = mx[k];
  }
  __syncthreads();
  int sh[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float all = red[k];
#pragma unroll
    for (int wv = 1; wv < kPpoAdamThreads / 64; ++wv) all = fmaxf(all, red[wv * 3 + k]);
    sh[k] = adam_shift(all);
  }

  // the fp16 section: 32 fragments x 64 lanes x 16 bytes, one 16-byte store per (fragment, lane)
  float* block = (actor ? a.actor_block : a.critic_block) + (size_t)g * kPolFloats;
  for (int q = t; q < kPolFrags * 64; q += kPpoAdamThreads) {
    const int frag = q >> 6, lane = q & 63, r = lane & 31, h = lane >> 5;
    int term, sft;
    float x[8];
    if (frag < kPolW2Frag) {                                       // layer 1: fragment (term*2 + mt)*2 + s, natural k order, k >= 17 zero
      term = frag >> 2; sft = sh[0];
      const int mt = (frag >> 1) & 1, s = frag & 1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 16 * s + 8 * h + j;
        x[j] = k < kPolIn ? w[kPpoW1 + (32 * mt + r) * kPolIn + k] : 0.0f;
      }
    } else {                                                       // layer 2: 8 + (term*2 + mt)*4 + ks; head: 24 + term*4 + ks, rows >= out_dim zero
      const bool head = frag >= kPolW3Frag;
      const int f = frag - (head ? kPolW3Frag : kPolW2Frag), ks = f & 3;
      term = head ? f >> 2 : f >> 3; sft = head ? sh[2] : sh[1];
      const int base = head ? kPpoW3 + r * kPolHid : kPpoW2 + (32 * ((f >> 2) & 1) + r) * kPolHid;
      const bool live = !head || r < out_dim;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
        x[j] = live ? w[base + k] : 0.0f;
      }
    }
    f16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ws = ldexpf(x[j], sft);
      const _Float16 hi = (_Float16)ws;                            // round to nearest even, subnormals kept
      out[j] = term == 0 ? hi : (_Float16)(ws - (float)hi);        // (the difference is exact in fp32)
    }
    *reinterpret_cast<f16x8*>(block + 4 * q) = out;
  }
  // the fp32 section: 180 floats, four per thread
  if (t < (kPolFloats - kPolF32) / 4) {
    float4 o;
    o.x = ppo_adam_tail(w, 4 * t + 0, actor, out_dim, sh[0], sh[1], sh[2]);
    o.y = ppo_adam_tail(w, 4 * t + 1, actor, out_dim, sh[0], sh[1], sh[2]);
    o.z = ppo_adam_tail(w, 4 * t + 2, actor, out_dim, sh[0], sh[1], sh[2]);
    o.w = ppo_adam_tail(w, 4 * t + 3, actor, out_dim, sh[0], sh[1], sh[2]);
    *reinterpret_cast<float4*>(block + kPolF32 + 4 * t) = o;
  }
}

// ---- every MLP architecture: the same two kernels on the layers of a table
static_assert(kPpoMlpAdamMaxFloats * 4 + 25 * 4 <= 64 * 1024, "the largest net's parameters fit the static LDS");

__global__ __launch_bounds__(kPpoAdamThreads) void ppo_mlp_adam_norm_kernel(const PpoMlpAdamLaunch A) {
  const PpoAdamLaunch& a = A.a;
  const int g = blockIdx.x, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (workgroup-uniform) an inactive member: nothing read, nothing written
  __shared__ double part[kPpoAdamThreads];
  const int na = A.T[0].grad_floats, nc = A.T[1].grad_floats;
  const float* ga = a.actor_grad + (size_t)g * na;
  const float* gc = a.critic_grad + (size_t)g * nc;
  double s = 0.0;
  for (int i = t; i < na + nc; i += kPpoAdamThreads) {
    const double x = (double)(i < na ? ga[i] : gc[i - na]);
    s += x * x;
  }
  part[t] = s;
  for (int w = kPpoAdamThreads / 2; w > 0; w >>= 1) {              // the fixed tree of ppo_adam_norm_kernel
    __syncthreads();
    if (t < w) part[t] += part[t + w];
  }
  if (t != 0) return;
  const float total = (float)sqrt(part[0]);
  float4* c = reinterpret_cast<float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (!(fabsf(total) <= 3.402823466e+38f)) {                       // inf or NaN: the member is skipped whole
    c[0] = make_float4(total, 0.0f, 0.0f, 0.0f);
    c[1] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float clip = (float)fmin(1.0, (double)a.max_grad_norm / ((double)total + (double)1e-6f));
  const int64_t tt = a.step[g] + 1;
  const double bc1 = 1.0 - pow(a.beta1, (double)tt), bc2 = 1.0 - pow(a.beta2, (double)tt);
  c[0] = make_float4(total, clip, (float)(a.lr / bc1), (float)(1.0 / sqrt(bc2)));
  c[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  a.step[g] = tt;
}

__global__ __launch_bounds__(kPpoAdamThreads) void ppo_mlp_adam_update_kernel(const PpoMlpAdamLaunch A) {
  const PpoAdamLaunch& a = A.a;
  const int net = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (both tests are workgroup-uniform and ahead of every barrier)
  const float4 c = *reinterpret_cast<const float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (a.coef[(size_t)g * kPpoAdamCoef + 4] != 0.0f) return;        // a non-finite norm: the member is skipped whole
  const float clip = c.y, step_size = c.z, isb2 = c.w;

  __shared__ __attribute__((aligned(16))) float w[kPpoMlpAdamMaxFloats];
  __shared__ float red[(kPpoAdamThreads / 64) * kMlpLayers];
  __shared__ int shs[kMlpLayers];
  const bool actor = net == 0;
  const PpoMlpTable& T = A.T[net];
  const int count = T.grad_floats, L = T.L;
  const size_t row = (size_t)g * (size_t)count;
  const float* gr = (actor ? a.actor_grad : a.critic_grad) + row;
  float* p = (actor ? a.actor_param : a.critic_param) + row;
  float* m = (actor ? a.actor_m : a.critic_m) + row;
  float* v = (actor ? a.actor_v : a.critic_v) + row;

  for (int i = t; i < count; i += kPpoAdamThreads) {
    const float gp = gr[i] * clip;
    const float mo = m[i];
    const float mn = mo + (gp - mo) * a.omb1;
    const float vn = v[i] * a.b2 + (a.omb2 * gp) * gp;
    const float pn = p[i] - step_size * (mn / (sqrtf(vn) * isb2 + a.eps));
    m[i] = mn; v[i] = vn; p[i] = pn;
    w[i] = pn;
  }
  __syncthreads();

  // max |w| per layer: the thread's, the wave's, the workgroup's (a maximum does not depend on the order)
  for (int l = 0; l <= L; ++l) {
    const int n = T.out_w[l] * T.in_w[l], at = T.w_off[l];
    float mx = 0.0f;
    for (int i = t; i < n; i += kPpoAdamThreads) mx = fmaxf(mx, fabsf(w[at + i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[(t >> 6) * kMlpLayers + l] = mx;
  }
  __syncthreads();
  if (t <= L) {
    float all = red[t];
#pragma unroll
    for (int wv = 1; wv < kPpoAdamThreads / 64; ++wv) all = fmaxf(all, red[wv * kMlpLayers + t]);
    shs[t] = adam_shift(all);
  }
  __syncthreads();

  float* block = (actor ? a.actor_block : a.critic_block) + (size_t)g * T.block_floats;
  int frags = 0, tiles = 0;
  for (int l = 0; l <= L; ++l) { frags += 2 * T.mt[l] * T.ks[l]; tiles += T.mt[l]; }

  // the fp16 section: one 16-byte store per (fragment, lane); fragment frag0_l + (term MT + mt) KS + ks of layer l
  for (int q = t; q < frags * 64; q += kPpoAdamThreads) {
    const int frag = q >> 6, lane = q & 63, r = lane & 31, h = lane >> 5;
    int l = 0, f0 = 0;
    for (int k = 0, at = 0; k <= L; ++k) {
      const int n = 2 * T.mt[k] * T.ks[k];
      if (frag >= at && frag < at + n) { l = k; f0 = at; }
      at += n;
    }
    const int MT = T.mt[l], KS = T.ks[l], in_w = T.in_w[l], out_w = T.out_w[l], at = T.w_off[l], sft = shs[l];
    const int f = frag - f0, term = f / (MT * KS), mt = (f / KS) % MT, ks = f % KS;
    const int orow = 32 * mt + r;
    f16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // layer 0: natural k order (its B operand is built from obs rows); later layers: the k order of an accumulator tile
      const int k = l == 0 ? 16 * ks + 8 * h + j : 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
      const float x = (orow < out_w && k < in_w) ? w[at + orow * in_w + k] : 0.0f;
      const float ws = ldexpf(x, sft);
      const _Float16 hi = (_Float16)ws;                            // round to nearest even, subnormals kept
      out[j] = term == 0 ? hi : (_Float16)(ws - (float)hi);        // (the difference is exact in fp32)
    }
    *reinterpret_cast<f16x8*>(block + kMlpHdr + 4 * q) = out;
  }
  // the biases in accumulator order, [mt][h][16] per layer, times the accumulator's scale; padded rows zero
  float* biases = block + kMlpHdr + frags * (kPolFragBytes / 4);
  for (int i = t; i < tiles * 32; i += kPpoAdamThreads) {
    const int tile = i >> 5;
    int l = 0, t0 = 0;
    for (int k = 0, at = 0; k <= L; ++k) {
      if (tile >= at && tile < at + T.mt[k]) { l = k; t0 = at; }
      at += T.mt[k];
    }
    const int mt = tile - t0, h = (i >> 4) & 1, e = i & 15;
    const int orow = 32 * mt + (e & 3) + 8 * (e >> 2) + 4 * h;
    biases[i] = orow < T.out_w[l] ? w[T.b_off[l] + orow] * ldexpf(1.0f, kPolXShift + shs[l]) : 0.0f;
  }
  // record word 4 of each layer: the inverse accumulator scale (a power of two: exact); an actor's exp(log_std) and log_std
  if (t <= L) block[kMlpRec + kMlpRecStride * t + 4] = ldexpf(1.0f, -(kPolXShift + shs[t]));
  if (actor && t >= 64 && t < 64 + kPolOut) {
    const float ls = w[T.ls_off + (t - 64)];
    block[kMlpStd + (t - 64)] = (float)exp((double)ls);
    block[kMlpStd + 8 + (t - 64)] = ls;
  }
}

void ppo_mlp_adam_launch(const PpoMlpAdamLaunch& A, hipStream_t s) {
  hipLaunchKernelGGL(ppo_mlp_adam_norm_kernel, dim3((unsigned)A.a.n_members), dim3(kPpoAdamThreads), 0, s, A);
  hipLaunchKernelGGL(ppo_mlp_adam_update_kernel, dim3(2, (unsigned)A.a.n_members), dim3(kPpoAdamThreads), 0, s, A);
}

void ppo_adam_launch(const PpoAdamLaunch& a, hipStream_t s) {
  hipLaunchKernelGGL(ppo_adam_norm_kernel, dim3((unsigned)a.n_members), dim3(kPpoAdamThreads), 0, s, a);
  hipLaunchKernelGGL(ppo_adam_update_kernel, dim3(2, (unsigned)a.n_members), dim3(kPpoAdamThreads), 0, s, a);
}

}  // namespace rdv

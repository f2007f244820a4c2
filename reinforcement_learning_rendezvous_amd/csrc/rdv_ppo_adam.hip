// rdv_ppo_adam.hip — the kernels of rdv_ppo_adam.h and their launch, in a translation unit of its own (the objects of the other units do
// not change when it does).  The exported rdv_ppo_set_adam_step and rdv_ppo_mlp_set_adam_step are in rdv_policy_host.hip, with the other
// policy entry points.
//
// The elementwise contract of include/rdv.h is float32 with every operation rounded on its own: nothing in this unit may be contracted
// into an fma.  `/` and sqrtf are hipcc's correctly rounded ones (its default; the v_fma of their expansions are theirs).
#pragma clang fp contract(off)
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy.h"
#include "rdv_policy_mlp.h"
#include "rdv_ppo_adam.h"

#include <type_traits>

namespace rdv {

// ---- the shipped block as a case of the layer table: the default spec's table, and where the two blocks keep what the update writes
constexpr RdvMlpSpec kAdamShippedSpec = {2, {kPolHid, kPolHid, 0, 0}, RDV_ACT_TANH, 0};
constexpr PpoMlpTable adam_shipped_table(bool actor) {
  PpoMlpTable t{};
  ppo_mlp_table(kAdamShippedSpec, actor, t);
  return t;
}
constexpr int adam_frags(const PpoMlpTable& t, int layers) {      // the fragments / the bias tiles of layers 0 .. layers - 1
  int n = 0;
  for (int l = 0; l < layers; ++l) n += 2 * t.mt[l] * t.ks[l];
  return n;
}
constexpr int adam_tiles(const PpoMlpTable& t, int layers) {
  int n = 0;
  for (int l = 0; l < layers; ++l) n += t.mt[l];
  return n;
}
// float indices inside a block: the fp16 section (the biases follow it), exp(log_std), log_std, layer l's inverse scale at scale + stride l
struct AdamBlockAt { int frags, std, log_std, scale, scale_stride; };
constexpr AdamBlockAt kAdamShippedAt = {0, kPolStd, kPolLogStd, kPolScale, 1};
constexpr AdamBlockAt kAdamMlpAt = {kMlpHdr, kMlpStd, kMlpStd + 8, kMlpRec + 4, kMlpRecStride};

constexpr bool adam_shipped_layout(bool actor) {
  const PpoMlpTable t = adam_shipped_table(actor);
  const int out_dim = actor ? kPolOut : 1;
  return t.L == 2 && t.w_off[0] == kPpoW1 && t.b_off[0] == kPpoB1 && t.w_off[1] == kPpoW2 && t.b_off[1] == kPpoB2 && t.w_off[2] == kPpoW3 &&
         t.b_off[2] == kPpoW3 + out_dim * kPolHid && t.grad_floats == (actor ? kPpoActorGrad : kPpoCriticGrad) &&
         t.ls_off == (actor ? kPpoActorGrad - kPolOut : -1) &&
         // the fragments [term][mt][ks] per layer from kPolW1Frag, kPolW2Frag, kPolW3Frag, the fp32 section right behind them
         adam_frags(t, 0) == kPolW1Frag && adam_frags(t, 1) == kPolW2Frag && adam_frags(t, 2) == kPolW3Frag && adam_frags(t, 3) == kPolFrags &&
         kPolF32 == kPolFrags * (kPolFragBytes / 4) &&
         // the biases [mt][h][16] per layer at kPolB1, kPolB2, kPolB3, then exp(log_std) [8], log_std [8], the scales [4]
         kPolB1 == kPolF32 && kPolB2 == kPolF32 + 32 * adam_tiles(t, 1) && kPolB3 == kPolF32 + 32 * adam_tiles(t, 2) &&
         kPolStd == kPolF32 + 32 * adam_tiles(t, 3) && kPolLogStd == kPolStd + 8 && kPolScale == kPolLogStd + 8 && kPolFloats == kPolScale + 4;
}
static_assert(adam_shipped_layout(true) && adam_shipped_layout(false), "the shipped block and RdvPpoOut's flat layouts are the default spec's row of the layer table");
static_assert(kPpoMlpAdamMaxFloats * 4 + 25 * 4 <= 64 * 1024 && kPpoActorGrad <= kPpoMlpAdamMaxFloats, "the largest net's parameters fit the static LDS");

// ---- 1. one norm, one clip coefficient and the two step coefficients per member
__global__ __launch_bounds__(kPpoAdamThreads) void ppo_adam_norm_kernel(const PpoAdamLaunch a) {
  const int g = blockIdx.x, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (workgroup-uniform) an inactive member: nothing read, nothing written
  __shared__ double part[kPpoAdamThreads];
  const int na = a.ga, nc = a.gc;
  const float* ga = a.actor_grad + (size_t)g * na;
  const float* gc = a.critic_grad + (size_t)g * nc;
  double s = 0.0;
  for (int i = t; i < na + nc; i += kPpoAdamThreads) {
    const double x = (double)(i < na ? ga[i] : gc[i - na]);
    s += x * x;                                                    // (the product of two floats is exact in double)
  }
  part[t] = s;
  for (int w = kPpoAdamThreads / 2; w > 0; w >>= 1) {              // a fixed tree: the order depends on the index alone
    __syncthreads();
    if (t < w) part[t] += part[t + w];
  }
  if (t == 0) adam_member_coef(a, g, part[0]);
}

// ---- 2. the step and the repack of one member's net.  SHIPPED: the arguments are the PpoAdamLaunch alone and the layers those of the
// default spec — ppo_mlp_table is constexpr and the spec a constant, so every entry is a literal or a select on the net, the layer loops
// unroll and the fragment arithmetic folds to shifts; otherwise the two tables travel in the arguments.
template <bool SHIPPED> using PpoAdamArgs = std::conditional_t<SHIPPED, PpoAdamLaunch, PpoMlpAdamLaunch>;
__host__ __device__ __forceinline__ const PpoAdamLaunch& ppo_adam_launch_of(const PpoAdamLaunch& A) { return A; }
__host__ __device__ __forceinline__ const PpoAdamLaunch& ppo_adam_launch_of(const PpoMlpAdamLaunch& A) { return A.a; }
__device__ __forceinline__ PpoMlpTable ppo_adam_table_of(const PpoAdamLaunch&, int net) { return adam_shipped_table(net == 0); }
__device__ __forceinline__ const PpoMlpTable& ppo_adam_table_of(const PpoMlpAdamLaunch& A, int net) { return A.T[net]; }

template <bool SHIPPED>
__global__ __launch_bounds__(kPpoAdamThreads) void ppo_adam_update_kernel(const PpoAdamArgs<SHIPPED> A) {
  const PpoAdamLaunch& a = ppo_adam_launch_of(A);
  const int net = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  if (!((a.mask >> g) & 1)) return;                                // (both tests are workgroup-uniform and ahead of every barrier)
  const float4 c = *reinterpret_cast<const float4*>(a.coef + (size_t)g * kPpoAdamCoef);
  if (a.coef[(size_t)g * kPpoAdamCoef + 4] != 0.0f) return;        // a non-finite norm: the member is skipped whole
  const float clip = c.y, step_size = c.z, isb2 = c.w;

  __shared__ __attribute__((aligned(16))) float w[SHIPPED ? kPpoActorGrad : kPpoMlpAdamMaxFloats];
  __shared__ float red[(kPpoAdamThreads / 64) * kMlpLayers];
  __shared__ int shs[kMlpLayers];
  constexpr AdamBlockAt at = SHIPPED ? kAdamShippedAt : kAdamMlpAt;
  const bool actor = net == 0;
  const auto& T = ppo_adam_table_of(A, net);
  const int count = T.grad_floats, L = T.L;
  const size_t row = (size_t)g * (size_t)count;
  const float* gr = (actor ? a.actor_grad : a.critic_grad) + row;
  float* p = (actor ? a.actor_param : a.critic_param) + row;
  float* m = (actor ? a.actor_m : a.critic_m) + row;
  float* v = (actor ? a.actor_v : a.critic_v) + row;

  for (int i = t; i < count; i += kPpoAdamThreads) {
    w[i] = adam_element(a, gr, m, v, p, i, clip, step_size, isb2);
  }
  __syncthreads();

  // max |w| per layer: the thread's, the wave's, the workgroup's (a maximum does not depend on the order)
  for (int l = 0; l <= L; ++l) {
    const int n = T.out_w[l] * T.in_w[l], at_w = T.w_off[l];
    float mx = 0.0f;
    for (int i = t; i < n; i += kPpoAdamThreads) mx = fmaxf(mx, fabsf(w[at_w + i]));
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

  float* block = (actor ? a.actor_block : a.critic_block) + (size_t)g * (SHIPPED ? kPolFloats : T.block_floats);
  // the fp16 section, layer by layer: one 16-byte store per (fragment, lane); fragment (term MT + mt) KS + ks of the layer's 2 MT KS
  float* out = block + at.frags;
  for (int l = 0; l <= L; ++l) {
    const int MT = T.mt[l], KS = T.ks[l], in_w = T.in_w[l], out_w = T.out_w[l], at_w = T.w_off[l], sft = shs[l];
    for (int q = t; q < 2 * MT * KS * 64; q += kPpoAdamThreads) {
      const int f = q >> 6, lane = q & 63, r = lane & 31, h = lane >> 5;
      const int term = f / (MT * KS), mt = (f / KS) % MT, ks = f % KS;
      const int orow = 32 * mt + r;
      f16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // layer 0: natural k order (its B operand is built from obs rows); later layers: the k order of an accumulator tile
        const int k = l == 0 ? adam_k_natural(ks, h, j) : adam_k_accumulator(ks, h, j);
        const float x = (orow < out_w && k < in_w) ? w[at_w + orow * in_w + k] : 0.0f;
        o[j] = adam_split_term(x, sft, term);
      }
      *reinterpret_cast<f16x8*>(out + 4 * q) = o;
    }
    out += 2 * MT * KS * (kPolFragBytes / 4);
  }
  // the biases in accumulator order, [mt][h][16] per layer, times the accumulator's scale; padded rows zero
  for (int l = 0; l <= L; ++l) {
    if (t < T.mt[l] * 32) {
      const int orow = adam_bias_row(t);
      out[t] = orow < T.out_w[l] ? w[T.b_off[l] + orow] * ldexpf(1.0f, kPolXShift + shs[l]) : 0.0f;
    }
    out += T.mt[l] * 32;
  }
  // each layer's inverse accumulator scale (a power of two: exact); an actor's exp(log_std) and log_std
  if (t <= L) block[at.scale + at.scale_stride * t] = ldexpf(1.0f, -(kPolXShift + shs[t]));
  if (actor && t >= 64 && t < 64 + kPolOut) {
    const float ls = w[T.ls_off + (t - 64)];
    block[at.std + (t - 64)] = (float)exp((double)ls);
    block[at.log_std + (t - 64)] = ls;
  }
}

template <bool SHIPPED>
static void adam_launch(const PpoAdamArgs<SHIPPED>& A, hipStream_t s) {
  const PpoAdamLaunch& a = ppo_adam_launch_of(A);
  hipLaunchKernelGGL(ppo_adam_norm_kernel, dim3((unsigned)a.n_members), dim3(kPpoAdamThreads), 0, s, a);
  hipLaunchKernelGGL(ppo_adam_update_kernel<SHIPPED>, dim3(2, (unsigned)a.n_members), dim3(kPpoAdamThreads), 0, s, A);
}
void ppo_adam_launch(const PpoAdamLaunch& a, hipStream_t s) { adam_launch<true>(a, s); }
void ppo_mlp_adam_launch(const PpoMlpAdamLaunch& A, hipStream_t s) { adam_launch<false>(A, s); }

}  // namespace rdv

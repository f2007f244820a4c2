// rdv_ppo_adam.h — the optimiser half of a sweep's update step (rdv_ppo_set_adam_step for the shipped actor and critic, include/rdv.h
// "Gradient clip, Adam and weight repack for policy sets"; rdv_ppo_mlp_set_adam_step for an actor set and a critic set of ANY pair of
// RdvMlpSpec, "... of every MLP architecture"): what SB3's PPO.train() does between `loss.backward()` and the next minibatch —
// clip_grad_norm_ over the policy's parameters, Adam, and (ours) the repack of the forward parameter blocks — on the device, for all P
// members of an actor set and a critic set at once.  The kernels are in rdv_ppo_adam.hip, a translation unit of its own; this header holds
// the sizes and the launches that the host unit (rdv_policy_host.hip) needs, and the description.
//
// ONE pair of kernels serves both calls: the layers of a net are a PpoMlpTable (rdv_ppo_mlp.h), and the shipped nets are the default
// spec's row of it.  Rows of the caller's arrays are Ga / Gc floats long (5708 / 5377, or rdv_ppo_mlp_grad_floats), back to back, hence
// 4-byte aligned only: every access to them is one float.  Two launches per call, both on the caller's stream:
//   1. ppo_adam_norm_kernel    grid (P), 256 threads.  Workgroup g, if bit g of the mask is set: the sum of squares of member g's
//      Ga + Gc gradient entries in double — thread t adds the entries t, t + 256, .. of the concatenation [actor | critic] in index
//      order, the 256 sums are added by a fixed tree — the square root in double, rounded to float once; clip_coef (in double from that float); with t = step[g] + 1
//      the two step coefficients in double, rounded to float once; coef[g]; step[g] <- t.  A norm that is not finite: coef[g][4] = 1 and
//      nothing else of the member changes, here or in the next kernel.
//   2. ppo_adam_update_kernel<SHIPPED>  grid (2, P), 256 threads.  Workgroup (net, g) owns member g's actor (net 0) or critic (net 1):
//        step    element i of the net's flat parameter vector (the layout of the gradients): g' = g clip_coef, m, v, p as the
//                header states them — float32, every operation rounded on its own (this unit is compiled with contraction off; the
//                division and the square root are the correctly rounded ones) — m, v and p go back to the caller's arrays and p stays in
//                LDS;
//        shifts  max |w| per layer over the LDS copy (a maximum has no order), then pol_layer_shift's rule;
//        repack  the forward block straight from LDS, layer by layer: thread q builds the 16 bytes that lane (q & 63) of the layer's
//                fragment (q >> 6) reads — fragment order [term][mt][ks], layer 0 in natural k order, later layers in the accumulator's;
//                eight weights gathered, scaled by 2^s, split into two fp16 terms with the hardware's round-to-nearest-even conversion
//                (v_cvt_f16_f32; fp16 and fp32 subnormals are kept: the kernel's float_denorm_mode is hipcc's default, 3 for both);
//                rows >= the layer's width and k >= its input width are zero, so a 16- or 32-wide layer's missing rows and k-steps, the
//                head's rows >= out_dim and layer 0's k >= 17 are zero fragments — then, behind the fragments, the biases in accumulator
//                order, [mt][h][16] per layer, times 2^(10 + s) (padded rows zero), each layer's inverse scale 2^-(10 + s), and an
//                actor's exp(log_std) (the double-precision exp rounded to float) and log_std.
//      The two instantiations are that one body; they differ in where the layers come from and in four float indices of the block:
//                                   SHIPPED (pack_policy_weights, rdv_policy.h)          general (pack_mlp_weights, rdv_policy_mlp.h)
//        layers                     the default spec's table, at compile time           the two PpoMlpTable, by value in the arguments
//        LDS copy of p              5708 floats: 22,832 B                               14,028 floats (4 x 64, actor): 56,112 B
//        the fp16 section starts    0                                                   kMlpHdr
//        exp(log_std)               kPolStd                                             kMlpStd
//        log_std                    kPolLogStd                                          kMlpStd + 8
//        inverse scale of layer l   kPolScale + l                                       kMlpRec + kMlpRecStride l + 4
//      (plus 20 maxima and 5 shifts of static LDS in both).  Only live floats are written: the shipped block's padding (std[6..7],
//      log_std[6..7], scale[3], a critic's sixteen std floats) and the general block's integer header, other record words and floats
//      64..127 are what the host packer wrote — zeros or constants of the spec — at creation and at every update_weights(), which
//      upload the whole block; nothing else writes a block.
//      The block is the host packer's byte for byte; exp(log_std) is the double-precision exp rounded to float on both sides (pol_std,
//      rdv_policy.h), two libraries' exp: held to 1 ulp, equal unless the two doubles straddle a float rounding boundary.
// No floating-point atomic, no workspace, nothing read from the forward blocks: the fp32 master weights are the caller's arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdv_ppo.h"
#include "rdv_ppo_mlp.h"

namespace rdv {

constexpr int kPpoAdamCoef = 8;        // total_norm, clip_coef, step_size, inv_sqrt_bc2, skipped, 0, 0, 0
constexpr int kPpoAdamThreads = 256;
constexpr int kPpoMlpAdamMaxFloats = 17 * 64 + 64 + 3 * (64 * 64 + 64) + 6 * 64 + 6 + 6;   // 14,028: the largest net's parameters

struct PpoAdamLaunch {
  float *actor_block, *critic_block;   // the sets' forward blocks (device; member g at g * the net's block floats)
  float *actor_param, *critic_param, *actor_m, *actor_v, *critic_m, *critic_v;   // [P,Ga] / [P,Gc]
  int64_t* step;                       // [P]
  float* coef;                         // [P,8]
  const float *actor_grad, *critic_grad;
  uint64_t mask;
  int32_t n_members, ga, gc;           // ga, gc: the row lengths (kPpoActorGrad / kPpoCriticGrad, or the tables' grad_floats)
  double lr, beta1, beta2;             // the step coefficients are taken in double on the device (they depend on step[g])
  float max_grad_norm, b1, b2, omb1, omb2, eps;   // each rounded from double once, on the host
};
inline PpoAdamLaunch ppo_adam_scalars(PpoAdamLaunch a, double lr, double beta1, double beta2, double eps, double max_grad_norm) {
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.max_grad_norm = (float)max_grad_norm; a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  return a;
}
struct PpoMlpAdamLaunch {
  PpoAdamLaunch a;
  PpoMlpTable T[2];                    // actor, critic
};
static_assert(sizeof(PpoMlpAdamLaunch) <= 4096, "the arguments fit the 4 KiB kernel-argument segment");

// ---- device pieces that the kernels of rdv_ppo_adam.hip and of rdv_ppo_lstm_adam.hip (the recurrent nets' step, rdv_ppo_lstm_adam.h) share.
// Both units are compiled with contraction off; every function here is inlined into its kernel.
// pol_layer_shift's rule on the layer's max |w|
__device__ __forceinline__ int adam_shift(float mx) {
  int sft = 10;
  while (sft > -20 && ldexpf(mx, sft) >= 32768.0f) --sft;
  return sft;
}
// member g's coefficients from its sum of squares (one thread of the member's norm workgroup): the square root in double, rounded to float
// once; a norm that is not finite flags the member and leaves step[g] alone
__device__ __forceinline__ void adam_member_coef(const PpoAdamLaunch& a, int g, double sumsq) {
  const float total = (float)sqrt(sumsq);
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
// the elementwise step of entry i of a net's rows (the four float32 lines of include/rdv.h) -> the new parameter
__device__ __forceinline__ float adam_element(const PpoAdamLaunch& a, const float* gr, float* m, float* v, float* p, int i, float clip, float step_size,
                                              float isb2) {
  const float gp = gr[i] * clip;
  const float mo = m[i];
  const float mn = mo + (gp - mo) * a.omb1;
  const float vn = v[i] * a.b2 + (a.omb2 * gp) * gp;
  const float pn = p[i] - step_size * (mn / (sqrtf(vn) * isb2 + a.eps));
  m[i] = mn; v[i] = vn; p[i] = pn;
  return pn;
}
// the input column that element j of lane half h of k-step ks of a weight fragment holds.  Natural order: a layer whose B operand is built
// from rows in memory (an MLP's layer 0, a recurrent trunk's layer 0, the LSTM cell); accumulator order: the k order of an accumulator tile
// used as the B operand (later layers).  (Two functions, the choice left to the kernel: as one function with the layer as an argument the
// instruction streams of ppo_adam_update_kernel change, profiles/lstm_adam_isa_diff.md.)
__device__ __forceinline__ int adam_k_natural(int ks, int h, int j) { return 16 * ks + 8 * h + j; }
__device__ __forceinline__ int adam_k_accumulator(int ks, int h, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }
// term 0 / 1 of the two-term fp16 split of x 2^sft
__device__ __forceinline__ _Float16 adam_split_term(float x, int sft, int term) {
  const float ws = ldexpf(x, sft);
  const _Float16 hi = (_Float16)ws;                                // round to nearest even, subnormals kept
  return term == 0 ? hi : (_Float16)(ws - (float)hi);              // (the difference is exact in fp32)
}
// the output row that float t of a layer's biases [mt][h][16] holds (accumulator order)
__device__ __forceinline__ int adam_bias_row(int t) { return 32 * (t >> 5) + (t & 3) + 8 * ((t & 15) >> 2) + 4 * ((t >> 4) & 1); }

__attribute__((visibility("hidden"))) void ppo_adam_launch(const PpoAdamLaunch& a, hipStream_t s);          // the shipped blocks
__attribute__((visibility("hidden"))) void ppo_mlp_adam_launch(const PpoMlpAdamLaunch& a, hipStream_t s);   // the blocks of a.T

}  // namespace rdv

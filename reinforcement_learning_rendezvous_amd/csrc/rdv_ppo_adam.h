// rdv_ppo_adam.h — the optimiser half of a sweep's update step for the shipped actor and critic (rdv_ppo_set_adam_step, include/rdv.h,
// "Gradient clip, Adam and weight repack for policy sets"): what SB3's PPO.train() does between `loss.backward()` and the next minibatch —
// clip_grad_norm_ over the policy's parameters, Adam, and (ours) the repack of the forward parameter blocks — on the device, for all P
// members of an actor set and a critic set at once.  The kernels are in rdv_ppo_adam.hip, a translation unit of its own; this header holds
// the sizes and the launch that the host unit (rdv_policy_host.hip) needs, and the description.
//
// Two launches per call, both on the caller's stream:
//   1. ppo_adam_norm_kernel    grid (P), 256 threads.  Workgroup g, if bit g of the mask is set: the sum of squares of member g's
//      5708 + 5377 gradient entries in double — thread t adds the entries t, t + 256, .. of the concatenation [actor | critic] in index
//      order, the 256 sums are added by a fixed tree — the square root in double, rounded to float once; clip_coef (in double from that float); with t = step[g] + 1
//      the two step coefficients in double, rounded to float once; coef[g]; step[g] <- t.  A norm that is not finite: coef[g][4] = 1 and
//      nothing else of the member changes, here or in the next kernel.
//   2. ppo_adam_update_kernel  grid (2, P), 256 threads.  Workgroup (net, g) owns member g's actor (net 0) or critic (net 1):
//        step    element i of the net's flat parameter vector (the layout of RdvPpoOut's gradients): g' = g clip_coef, m, v, p as the
//                header states them — float32, every operation rounded on its own (this unit is compiled with contraction off; the
//                division and the square root are the correctly rounded ones) — m, v and p go back to the caller's arrays and p stays in
//                LDS (5708 floats: 22,832 B);
//        shifts  max |w| per layer over the LDS copy (a maximum has no order), then pol_layer_shift's rule;
//        repack  the 33,488 B forward block of rdv_policy.h straight from LDS: thread q of 2048 builds the 16 bytes that lane (q & 63) of
//                fragment (q >> 6) reads — eight weights gathered in the fragment's k order, scaled by 2^s, split into two fp16 terms with
//                the hardware's round-to-nearest-even conversion (v_cvt_f16_f32; fp16 and fp32 subnormals are kept: the kernel's
//                float_denorm_mode is hipcc's default, 3 for both) — and 45 more threads the fp32 section (biases in accumulator order times 2^(10 + s),
//                exp(log_std), log_std, the inverse scales, the padding), all with 16-byte stores.
//      The block is pack_policy_weights' byte for byte but for exp(log_std): the host takes libm's expf, the device the double-precision
//      exp rounded to float.
// No floating-point atomic, no workspace, nothing read from the forward blocks: the fp32 master weights are the caller's arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdv_ppo.h"
#include "rdv_ppo_mlp.h"

namespace rdv {

constexpr int kPpoAdamCoef = 8;        // total_norm, clip_coef, step_size, inv_sqrt_bc2, skipped, 0, 0, 0
constexpr int kPpoAdamThreads = 256;

struct PpoAdamLaunch {
  float *actor_block, *critic_block;   // the sets' forward blocks (device; member g at g * kPolFloats)
  float *actor_param, *critic_param, *actor_m, *actor_v, *critic_m, *critic_v;   // [P,5708] / [P,5377]
  int64_t* step;                       // [P]
  float* coef;                         // [P,8]
  const float *actor_grad, *critic_grad;
  uint64_t mask;
  int32_t n_members;
  double lr, beta1, beta2;             // the step coefficients are taken in double on the device (they depend on step[g])
  float max_grad_norm, b1, b2, omb1, omb2, eps;   // each rounded from double once, on the host
};
inline PpoAdamLaunch ppo_adam_scalars(PpoAdamLaunch a, double lr, double beta1, double beta2, double eps, double max_grad_norm) {
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.max_grad_norm = (float)max_grad_norm; a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  return a;
}

__attribute__((visibility("hidden"))) void ppo_adam_launch(const PpoAdamLaunch& a, hipStream_t s);

// ---- every MLP architecture (rdv_ppo_mlp_set_adam_step, include/rdv.h "Gradient clip, Adam and weight repack for policy sets of every
// MLP architecture"): the same two launches for an actor set and a critic set of ANY pair of RdvMlpSpec, the layers taken from the two
// PpoMlpTable (rdv_ppo_mlp.h) that travel by value in the kernel arguments.  Rows are Ga / Gc floats long (rdv_ppo_mlp_grad_floats), back
// to back, hence 4-byte aligned only: every access to them is one float.
//   1. ppo_mlp_adam_norm_kernel    grid (P): ppo_adam_norm_kernel with the two lengths as arguments — the same double sums (thread t adds
//      entries t, t + 256, .. of [actor | critic], the fixed tree), the same coefficients, the same skip of a non-finite norm.
//   2. ppo_mlp_adam_update_kernel  grid (2, P), 256 threads, workgroup (net, g):
//        step    the four float32 lines of ppo_adam_update_kernel; the new parameters stay in LDS: 14,028 floats for the largest net
//                (4 x 64, actor) = 56,112 B, plus 20 maxima and 5 shifts: 56,212 B static LDS;
//        shifts  max |w| per layer, then pol_layer_shift's rule;
//        repack  the forward block of pack_mlp_weights (rdv_policy_mlp.h) from LDS: thread q builds the 16 bytes that lane (q & 63) of
//                fragment (q >> 6) reads — fragment order [term][mt][ks] per layer, layer 0 in natural k order, later layers in the
//                accumulator's; rows >= the layer's width and k >= its input width are zero, so a 16- or 32-wide layer's missing rows
//                and k-steps and the head's rows >= out_dim are zero fragments — then the biases in accumulator order times
//                2^(10 + s) (padded rows zero), record word 4 of each layer (2^-(10 + s)), and an actor's exp(log_std) (the
//                double-precision exp rounded to float) and log_std.  The block's integer header, the other record words and floats
//                64..127 are constants of the spec: they are left as rdv_policy_set_create wrote them.
// The shipped kernels above stay as they are beside these (their instruction streams are the parent's: profiles/ppo_mlp_set_isa_diff.md);
// the shipped block's layout (biases before the scales, no header) is another one, not a case of this table.
constexpr int kPpoMlpAdamMaxFloats = 17 * 64 + 64 + 3 * (64 * 64 + 64) + 6 * 64 + 6 + 6;   // 14,028
struct PpoMlpAdamLaunch {
  PpoAdamLaunch a;                 // the blocks: member g at g * T[net].block_floats; the rows [P, Ga] / [P, Gc]
  PpoMlpTable T[2];                // actor, critic
};
static_assert(sizeof(PpoMlpAdamLaunch) <= 4096, "the arguments fit the 4 KiB kernel-argument segment");
__attribute__((visibility("hidden"))) void ppo_mlp_adam_launch(const PpoMlpAdamLaunch& a, hipStream_t s);

}  // namespace rdv

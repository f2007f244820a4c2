// rdv_ppo.h — the PPO minibatch loss and its gradients for the shipped actor and critic (rdv_ppo_loss_grad, include/rdv.h, "PPO minibatch
// gradients"): what SB3's PPO.train() computes for ONE minibatch between `rollout_buffer.get` and `optimizer.step`, on the device.
// The kernels are in rdv_ppo.hip, a translation unit of its own; this header holds the sizes and the launch that the host unit
// (rdv_policy_host.hip) needs, and the description.
//
// Four launches per call, all on the caller's stream:
//   1. ppo_transpose_kernel: the A-operand fragments of W3^T and W2^T of both nets, derived from the handles' FORWARD blocks (a permutation
//      of their fp16 terms: (hi + lo) 2^-s is exactly the weight the forward pass multiplies by, i.e. the function being differentiated)
//      into the head of the workspace.  No host state is added to the handles; a call enqueued behind rdv_policy_set_weights reads the new block.
//   2. ppo_net_kernel<true, false>  (actor)  and  3. ppo_net_kernel<false, false> (critic): a wave owns 32 minibatch rows, a workgroup 256, as in
//      policy_act_kernel.  Per wave:
//        gather   the rows' observations by `indices` into the wave's LDS rows (68-byte rows, as stage_obs_rows stages contiguous ones);
//        forward  the shipped device functions of rdv_policy.h (actor_inputs, layer, tanh2_f32, split2: the sequence of actor_means, so
//                 the means and the values are the bits of rdv_policy_act / rdv_policy_value), keeping h1 and h2 (times 2^10) in registers;
//        loss     per lane: log_prob, ratio, the clip rule, d loss / d mean_c and d loss / d log_std_c (actor), 2 vf_coef (v - return) (critic),
//                 WITHOUT the 1/n of the means (the last kernel divides);
//        backward delta_{l-1} = (W_l^T delta_l) o (1 - h_{l-1}^2): the forward's `layer` with the transposed fragments as A operand and the
//                 error tile — an accumulator tile again — as B operand;
//        weights  dW_l = delta_l h_{l-1}^T contracted over the wave's 32 rows (k = rows): both operands need the row index along k, so
//                 delta_l and h_{l-1} are transposed through the wave's LDS tiles ([term][feature][row] fp16); the bias gradients (and
//                 d log_std) are one more column tile of ones.
//      Every backward operand is brought to fp32 level as the forward's: scaled by a power of two (here the WAVE's: the largest |delta| of
//      the tile goes to [2^13, 2^14)), split into two fp16 terms, three MFMAs per product (mfma3).  The per-wave tiles are added in LDS in
//      wave order and the workgroup's sums go to its row of the workspace: no floating-point atomic anywhere, the same bits every time.
//   4. ppo_finish_kernel: adds the workgroups' rows in index order, divides by n, adds the entropy term to d log_std, writes actor_grad,
//      critic_grad and the eight scalars.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdv {

constexpr int kPpoActorGrad = 5708;    // w1[64,17] b1[64] w2[64,64] b2[64] w3[6,64] b3[6] log_std[6]
constexpr int kPpoCriticGrad = 5377;   // w1 b1 w2 b2 w3[1,64] b3[1]
constexpr int kPpoScalars = 8;
constexpr int kPpoW1 = 0, kPpoB1 = 1088, kPpoW2 = 1152, kPpoB2 = 5248, kPpoW3 = 5312;   // offsets inside either gradient; b3 = w3 + out_dim * 64
// backward block of one net: 20 fragments of 1 KiB ([q][mt][ks]: W3^T at 0 (2 x 2 x 1), W2^T at 4 (2 x 2 x 4)), then 64 zero floats (the
// "bias" that `layer` starts its accumulators from)
constexpr int kPpoBwdW3 = 0, kPpoBwdW2 = 4, kPpoBwdFrags = 20;
constexpr int kPpoBwdZero = kPpoBwdFrags * 256, kPpoBwdFloats = kPpoBwdZero + 64;       // 5,184 floats = 20,736 B
// a workgroup's row of partial sums: actor gradient | critic gradient | (pad to 16 bytes) | policy, kl, clipped count, value sums
constexpr int kPpoPartCritic = kPpoActorGrad, kPpoPartScalars = 11088, kPpoPartFloats = 11096;
static_assert(kPpoPartCritic + kPpoCriticGrad <= kPpoPartScalars, "the scalar sums lie behind the critic's gradient");
constexpr int kPpoBlockRows = 256;     // kPolBlockEnvs

inline int64_t ppo_workgroups(int64_t n) { return (n + kPpoBlockRows - 1) / kPpoBlockRows; }
inline int64_t ppo_workspace_bytes(int64_t n) { return (2 * (int64_t)kPpoBwdFloats + ppo_workgroups(n) * kPpoPartFloats) * (int64_t)sizeof(float); }

// the coefficients of a call as the kernels take them, from the entry points' doubles: the clip limits' differences are taken in double
struct PpoCoefs { float clip_lo, clip_hi, clip_range, ent_coef, vf_coef; };
inline PpoCoefs ppo_coefs(double eps, double ent_coef, double vf_coef) { return {(float)(1.0 - eps), (float)(1.0 + eps), (float)eps, (float)ent_coef, (float)vf_coef}; }

struct PpoLaunch {
  const float *actor_block, *critic_block;   // the handles' forward parameter blocks (device)
  const float *obs, *actions, *old_log_prob, *advantages, *returns;
  const int64_t* indices;                    // nullable
  int64_t n;
  PpoCoefs k;
  float* workspace;
  float *actor_grad, *critic_grad, *scalars, *log_prob, *values;
};

// ---- the set form (rdv_ppo_set_loss_grad, include/rdv.h "PPO minibatch gradients for policy sets"): P members' minibatches in the same
// four launches, as rdv_policy_sets.h gives the forward kernels a set form — the same bodies, the member taken from the grid.
//   ppo_set_transpose_kernel  grid (21, 2, P)                        member z, net y
//   ppo_net_kernel<A, true>   grid (max_g workgroups(counts[g]), P)  workgroup (x, y) is workgroup x of member y's stand-alone launch; it
//                             returns before its first barrier when x >= workgroups(counts[y]) (a workgroup-uniform test)
//   ppo_set_finish_kernel     grid (44, P)                           member y
// Everything a workgroup touches is the stand-alone kernel's, offset by member: the forward block is set base + y * kPolFloats (the set
// allocation holds exactly the bytes of stand-alone handles), the backward blocks and `parts` are member y's piece of the workspace,
// `indices`, log_prob and values are advanced by off[y], n is count[y].  wave_base, the LDS layout, the wave-order sums and the index-order
// sum of the last kernel are per member exactly as alone, so every output of member y has the bits of the stand-alone call.
// count, off and the workspace offsets travel BY VALUE in the kernel arguments (PpoSetTable): no device table, hence no host-to-device
// copy that a capture would forbid.  That is the reason for the cap: 64 members x 3 x 8 bytes = 1,536 B of the 4 KiB argument segment, next
// to the 104 B of the stand-alone kernel's own arguments.
// The workspace, member after member, members with count 0 left out: [2 x kPpoBwdFloats | workgroups(count[g]) x kPpoPartFloats] floats;
// both pieces are multiples of 16 bytes.
constexpr int kPpoSetMaxMembers = 64;
struct PpoSetTable {
  int64_t count[kPpoSetMaxMembers];   // member g's minibatch size (0: the member takes no part)
  int64_t off[kPpoSetMaxMembers];     // count[0] + .. + count[g-1]: where its indices, log_prob and values start
  int64_t ws[kPpoSetMaxMembers];      // where its piece of the workspace starts, in floats
};
static_assert((2 * kPpoBwdFloats) % 4 == 0 && kPpoPartFloats % 4 == 0, "every piece of the workspace is 16-byte aligned");
// fills `t` for counts[0 .. n_members) (all >= 0, n_members <= kPpoSetMaxMembers) -> the workspace's size in bytes
inline int64_t ppo_set_table(int32_t n_members, const int64_t* counts, PpoSetTable* t, int64_t* total = nullptr, int64_t* max_workgroups = nullptr) {
  int64_t off = 0, ws = 0, most = 0;
  for (int g = 0; g < kPpoSetMaxMembers; ++g) {
    const int64_t c = g < n_members ? counts[g] : 0;
    if (t) { t->count[g] = c; t->off[g] = off; t->ws[g] = ws; }
    off += c;
    if (c > 0) ws += 2 * (int64_t)kPpoBwdFloats + ppo_workgroups(c) * kPpoPartFloats;
    if (ppo_workgroups(c) > most) most = ppo_workgroups(c);
  }
  if (total) *total = off;
  if (max_workgroups) *max_workgroups = most;
  return ws * (int64_t)sizeof(float);
}

struct PpoSetLaunch {
  PpoLaunch a;            // actor_block, critic_block: the sets' allocations (member g at g * kPolFloats); n unused; indices required;
                          // actor_grad [P,5708], critic_grad [P,5377], scalars [P,8]; log_prob, values [sum of counts], nullable
  int32_t n_members;
  int64_t max_workgroups;
  PpoSetTable table;
};

__attribute__((visibility("hidden"))) hipError_t ppo_raise_lds_limit();   // the plain and the set instantiations
__attribute__((visibility("hidden"))) void ppo_launch(const PpoLaunch& a, hipStream_t s);
__attribute__((visibility("hidden"))) void ppo_set_launch(const PpoSetLaunch& a, hipStream_t s);

}  // namespace rdv

// rdv_policy_mlp.h — the actor and critic of rdv_policy.h for the other architectures of the reference's network sweep
// (tune_policy.py:30-34, :124-139; custom/custom_networks.py:9-10): 1..4 hidden layers, each 16, 32 or 64 wide, one activation out
// of tanh / ReLU / sigmoid for the whole network (RdvMlpSpec, include/rdv.h).  The scheme is rdv_policy.h's, with its functions:
// power-of-two scaling, two fp16 terms per operand (split2), three v_mfma_f32_32x32x16_f16 per k-step (mfma3), transposed layers
// (layer<MT, KS>), the accumulator tile as the next layer's B operand in the permuted k order, observation and action rows staged
// through LDS (stage_obs_rows, actor_inputs, actor_outputs), the same noise (actor_noise, actor_apply_at, clip_action).
//
// Widths on tiles.  A layer of width 64 is two 32-row tiles (MT = 2) and gives the next layer four k-steps; 32 is one tile and two
// k-steps; 16 is one tile whose rows 16..31 have zero weights and a zero bias, and ONE k-step: rows 0..15 of a tile are registers
// 0..7 of both lane halves ((e & 3) + 8 (e >> 2) + 4 h), exactly the fragment of k-step 0, so the next layer is packed with one
// k-step and never reads the padded rows (whose activations are not zero: sigmoid(0) = 0.5).
//
// Structure.  ONE loop over the hidden layers (the 17 inputs are the two k-steps of layer 0), its body a wave-uniform switch over the
// six (MT, KS) shapes, each fully unrolled on register arrays with constant indices; then the head, a switch over KS.  The kernels
// are templates on the activation and on actor / critic only: six instantiations, not one per architecture.  The layer table
// (fragment index, bias offset, MT, KS, inverse scale per layer) is the head of the parameter block and is read with scalar loads.
//
// Parameter block and LDS.  The whole block goes to LDS once per workgroup, as in rdv_policy.h; its size follows the network:
//   floats = 128 (layer table, exp(log_std), log_std, 64 zeros) + 256 F (F weight fragments of 1 KiB: 2 MT KS per layer) + 32 T (T tiles of biases)
// and the workgroup's dynamic LDS is that plus the 23,552 B of the eight waves' observation and action rows.  [32, 32]: F = 12,
// 36,736 B, four workgroups of 8 waves per CU by LDS; the shipped 64-64: F = 32, 57,472 B, two; 3 x 64: F = 48, 74,112 B, two;
// 4 x 64, the largest: F = 64, 90,752 B, ONE workgroup (two waves per SIMD) of the CU's 160 KiB.  hipFuncAttributeMaxDynamicShared-
// MemorySize of the six kernels is raised to that maximum (kMlpMaxLdsBytes) when the first handle is created.
//
// Biases.  rdv_policy.h starts a layer's accumulator from the (scaled) bias; here the accumulator starts from ZERO (layer<> is given
// the block's 64 zeros as its bias rows) and the bias is added behind the last MFMA.  The accumulator is rounded after every MFMA
// (3 per k-step, up to 12 per layer), each time at the magnitude it has THEN: started from a bias that is large against the sum —
// a head bias of 0.9 over products that add up to 0.05, a hidden ReLU bias of 3 — every one of those roundings is half an ulp of
// the bias, and they add up to several ulps of the result (measured on an MI355X, [64] ReLU with such biases, bias first: 3.1e-7 at an output of 0.9, where
// a float32 evaluation is within 3.7e-8).  Summing the products first and adding the bias once rounds at the bias's magnitude
// once, as a float32 GEMM + bias does.
//
// Activations, fp32 in registers on the scaled accumulator, the accumulator's scale folded into the constant, the result times 2^10:
//   tanh     tanh2_f32 of rdv_policy.h (absolute error <= 2.5e-7).
//   sigmoid  1 / (1 + 2^(-x log2 e)) on v_exp_f32 and v_rcp_f32 (1 ulp each).  Absolute error <= kMlpSigmoidAbsErr = 2.0e-7:
//            with u = 2^-23, the argument y = x * (-log2 e) carries a relative error of u (the product's and the constant's
//            rounding, 2^-24 each), i.e. e = 2^y a relative error of |x| u, plus v_exp_f32's u: (|x| + 1) u; d sigma / d e * e =
//            -sigma (1 - sigma), so that part is sigma (1 - sigma) (|x| + 1) u.  The sum 1 + e rounds (u / 2) and v_rcp_f32 adds u,
//            both relative to the result: 1.5 sigma u.  The maximum over x of sigma (1 - sigma) (|x| + 1) + 1.5 sigma is 1.64 (at
//            x ~ 2.3), times u = 1.96e-7.  x << 0: e = inf, the result is exactly 0; x >> 0: e = 0, exactly 1; NaN stays NaN.
//            No larger than tanh's bound.
//   ReLU     exact: the accumulator times a power of two, clamped to [0, 63] — the scaled fp16 terms of the next layer's operand
//            hold 63 * 2^10 and not more, the reason for the +-63 clamp of the inputs (rdv.h: the second deviation from the PyTorch
//            modules).  v_max_f32 / v_med3_f32 return a number for a NaN, so the NaN is selected explicitly, as clip_action does.
#pragma once

#include "rdv_policy.h"
#include "../../include/rdv.h"

namespace rdv {

constexpr float kMlpSigmoidAbsErr = 2.0e-7f;                     // derived above; tests/policy_mlp_reference.py uses this number
constexpr int kMlpLayers = RDV_MLP_MAX_HIDDEN + 1;               // hidden layers + head
// block: int words 0..3 = n_hidden, activation, out_dim, floats of the block; per layer l a record of 8 words from 8 + 8 l:
// first fragment, float offset of the biases, MT, KS, inverse accumulator scale 2^-(10 + s_l) (float); floats 48..55 exp(log_std),
// 56..63 log_std (rdv_policy.h's order from kPolStd on); floats 64..127 zero (the accumulators' initial value); fragments from float
// 128 ([q][mt][ks] per layer, as there); then the biases in accumulator order, [mt][h][16] per layer.
constexpr int kMlpRec = 8, kMlpRecStride = 8, kMlpStd = 48, kMlpZero = 64, kMlpHdr = 128;
static_assert(kPolLogStd - kPolStd == 8, "actor_apply_at reads log_std 8 floats behind exp(log_std)");
constexpr int kMlpStageFloats = (kPolBlock / 64) * (kPolObsStage + kPolActStage);
constexpr int kMlpMaxFloats = kMlpHdr + (8 + 3 * 16 + 8) * (kPolFragBytes / 4) + (4 * 2 + 1) * 32;
constexpr int kMlpMaxLdsBytes = (kMlpMaxFloats + kMlpStageFloats) * 4;   // 90,752 B
static_assert(kMlpMaxLdsBytes <= 160 * 1024, "the largest network's workgroup must fit the CU's 160 KiB of LDS");
inline int mlp_lds_bytes(int block_floats) { return (block_floats + kMlpStageFloats) * 4; }

constexpr int mlp_tiles(int width) { return width == 64 ? 2 : 1; }
constexpr int mlp_ksteps(int width) { return width / 16; }           // 16 -> 1, 32 -> 2, 64 -> 4

// Host: the parameter block of a network of `spec` (checked by the caller) with out_dim <= 6 output rows; weights[l] / biases[l] in
// SB3's layout, hidden layers first, the head last.  Scaling, splitting and fragment order are pack_policy_weights'.
inline void pack_mlp_weights(const RdvMlpSpec& spec, int out_dim, const float* const* weights, const float* const* biases,
                             const float* log_std, std::vector<float>& packed) {
  const int L = spec.n_hidden;
  int frag0[kMlpLayers], mt_n[kMlpLayers], ks_n[kMlpLayers], in_w[kMlpLayers], out_w[kMlpLayers], frags_total = 0, tiles_total = 0;
  for (int l = 0; l <= L; ++l) {
    in_w[l] = l == 0 ? kPolIn : spec.hidden[l - 1];
    out_w[l] = l < L ? spec.hidden[l] : out_dim;
    mt_n[l] = l < L ? mlp_tiles(out_w[l]) : 1;
    ks_n[l] = l == 0 ? 2 : mlp_ksteps(in_w[l]);
    frag0[l] = frags_total;
    frags_total += 2 * mt_n[l] * ks_n[l];
    tiles_total += mt_n[l];
  }
  const int bias0 = kMlpHdr + frags_total * (kPolFragBytes / 4);
  const int total = bias0 + tiles_total * 32;
  packed.assign((size_t)total, 0.0f);
  int32_t* hdr = reinterpret_cast<int32_t*>(packed.data());
  hdr[0] = L; hdr[1] = spec.activation; hdr[2] = out_dim; hdr[3] = total;
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
            // layer 0: natural k order (its B operand is built from obs rows); later layers: the k order of an accumulator tile
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
  if (log_std) for (int j = 0; j < out_dim; ++j) { packed[kMlpStd + j] = pol_std(log_std[j]); packed[kMlpStd + 8 + j] = log_std[j]; }
}

// The launches (rdv_policy_mlp.hip: the kernels have a translation unit of their own, so rdv_hip.hip's objects stay what they were).
hipError_t mlp_raise_lds_limit();
void mlp_launch_act(int activation, const float* W, int block_floats, const float* obs, float* actions, int64_t n, int deterministic,
                    uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s);
void mlp_launch_value(int activation, const float* W, int block_floats, const float* obs, float* values, int64_t n, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------- device
// the constant that takes a layer's scaled accumulator to its activation's argument (inv = 2^-(10 + s_layer), exact)
template <int ACT>
__device__ __forceinline__ float mlp_act_const(float inv) {
  if (ACT == RDV_ACT_TANH) return 2.8853900817779268f * inv;              // 2 log2 e
  if (ACT == RDV_ACT_SIGMOID) return -1.4426950408889634f * inv;          // -log2 e
  return inv * (float)(1 << kPolXShift);                                   // ReLU: the rescaling itself
}

// two activations of scaled accumulator values; the results leave times 2^10
template <int ACT>
__device__ __forceinline__ void mlp_act2(float x0, float x1, float k, float& t0, float& t1) {
  constexpr float one = (float)(1 << kPolXShift);
  if (ACT == RDV_ACT_TANH) {
    tanh2_f32(x0, x1, k, t0, t1);
  } else if (ACT == RDV_ACT_SIGMOID) {
    const pol_f2 y = pol_f2{x0, x1} * k;
    const pol_f2 e = {__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
    const pol_f2 s1 = e + 1.0f;
    const pol_f2 r = {__builtin_amdgcn_rcpf(s1.x), __builtin_amdgcn_rcpf(s1.y)};
    const pol_f2 t = r * one;
    t0 = t.x; t1 = t.y;
  } else {
    const pol_f2 v = pol_f2{x0, x1} * k;
    const float c0 = __builtin_amdgcn_fmed3f(v.x, 0.0f, 63.0f * one), c1 = __builtin_amdgcn_fmed3f(v.y, 0.0f, 63.0f * one);
    t0 = v.x != v.x ? v.x : c0; t1 = v.y != v.y ? v.y : c1;                // NaN stays NaN
  }
}

// activation of a (scaled) accumulator tile, split into the B fragments of the next layer's k-steps 2 t, 2 t + 1
template <int ACT>
__device__ __forceinline__ void mlp_activate(const f32x16& d, float k, f16x8 (&lo_step)[2], f16x8 (&hi_step)[2]) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; j += 2) mlp_act2<ACT>(d[j], d[j + 1], k, x[j], x[j + 1]);
  split2(x, lo_step);
#pragma unroll
  for (int j = 0; j < 8; j += 2) mlp_act2<ACT>(d[8 + j], d[9 + j], k, x[j], x[j + 1]);
  split2(x, hi_step);
}

// the (scaled) bias of this lane's 16 rows of a tile, added behind the products (see "Biases" above)
__device__ __forceinline__ void mlp_add_bias(f32x16& d, const float* b16) {
#pragma unroll
  for (int e4 = 0; e4 < 4; ++e4) {
    const float4 b = *reinterpret_cast<const float4*>(b16 + 4 * e4);
    d[4 * e4 + 0] += b.x; d[4 * e4 + 1] += b.y; d[4 * e4 + 2] += b.z; d[4 * e4 + 3] += b.w;
  }
}

// one hidden layer of MT tiles over KS k-steps: x (the B fragments of its input) becomes the B fragments of its output
template <int ACT, int MT, int KS>
__device__ __forceinline__ void mlp_hidden(const float* wf, const float* zerop, int frag0, const float* biasp, float k, int lane, f16x8 (&x)[4][2]) {
  f16x8 xin[KS][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) { xin[ks][0] = x[ks][0]; xin[ks][1] = x[ks][1]; }
  f32x16 d[MT];
  layer<MT, KS>(wf, frag0, zerop, xin, lane, d);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mlp_add_bias(d[mt], biasp + (mt * 2 + (lane >> 5)) * 16);
    mlp_activate<ACT>(d[mt], k, x[2 * mt], x[2 * mt + 1]);
  }
}

template <int KS>
__device__ __forceinline__ void mlp_head(const float* wf, const float* zerop, int frag0, const float* biasp, float inv, int lane, const f16x8 (&x)[4][2], float (&mean)[4]) {
  f16x8 xin[KS][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) { xin[ks][0] = x[ks][0]; xin[ks][1] = x[ks][1]; }
  f32x16 d[1];
  layer<1, KS>(wf, frag0, zerop, xin, lane, d);
  const float4 b = *reinterpret_cast<const float4*>(biasp + (lane >> 5) * 16);   // rows (e & 3) + 4 h, e < 4, of the head's bias rows
  d[0][0] += b.x; d[0][1] += b.y; d[0][2] += b.z; d[0][3] += b.w;
  mean[0] = d[0][0] * inv; mean[1] = d[0][1] * inv; mean[2] = d[0][2] * inv; mean[3] = d[0][3] * inv;   // rows (e & 3) + 4 h
}

// The network for the wave's 32 envs; the outputs as actor_means gives them.  `w`: the block in LDS; `H`: the same block in device
// memory, whose layer table is read with scalar loads (wave-uniform: every branch below is).
template <int ACT>
__device__ __forceinline__ void mlp_means(const float* w, const int32_t* __restrict__ H, const float* rows, int lane, float (&mean)[4]) {
  const float* wf = w + kMlpHdr;
  const float* zerop = w + kMlpZero;
  const int L = H[0];
  f16x8 x[4][2];
  {
    f16x8 x0[2][2];
    actor_inputs(rows, lane, x0);
#pragma unroll
    for (int q = 0; q < 2; ++q) { x[0][q] = x0[0][q]; x[1][q] = x0[1][q]; x[2][q] = (f16x8)(0); x[3][q] = (f16x8)(0); }
  }
#pragma nounroll
  for (int l = 0; l < L; ++l) {
    const int32_t* rec = H + kMlpRec + kMlpRecStride * l;
    const int frag0 = rec[0];
    const float* biasp = w + rec[1];
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
  const int32_t* rec = H + kMlpRec + kMlpRecStride * L;
  const int frag0 = rec[0];
  const float* biasp = w + rec[1];
  const float inv = __int_as_float(rec[4]);
  switch (rec[3]) {
    case 1: mlp_head<1>(wf, zerop, frag0, biasp, inv, lane, x, mean); break;
    case 2: mlp_head<2>(wf, zerop, frag0, biasp, inv, lane, x, mean); break;
    default: mlp_head<4>(wf, zerop, frag0, biasp, inv, lane, x, mean); break;
  }
}

// policy_act_kernel / policy_value_kernel of rdv_policy.h for a block of pack_mlp_weights.  Four waves per SIMD asked for (two workgroups
// per CU where the LDS allows): without it two instantiations took 130 registers, one workgroup per CU; with it 113-128, no scratch.  CRITIC: out = values [n], the noise
// arguments and raw_actions / log_prob are not used; otherwise out = actions [n,6].
template <int ACT, bool CRITIC>
__global__ __launch_bounds__(kPolBlock) __attribute__((amdgpu_waves_per_eu(4))) void mlp_kernel(const float* __restrict__ W, const float* __restrict__ obs, float* __restrict__ out,
                                                        int64_t n, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset,
                                                        float* __restrict__ raw_actions, float* __restrict__ log_prob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [parameters][8 x obs rows][8 x action rows]
  const int32_t* H = reinterpret_cast<const int32_t*>(W);
  const int total = H[3];
  float* w = lds;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  float* rows = lds + total + wv * kPolObsStage;
  float* arows = lds + total + (kPolBlock / 64) * kPolObsStage + wv * kPolActStage;
  const int64_t wave_base = ((int64_t)blockIdx.x * (kPolBlock / 64) + wv) * kPolWaveEnvs;
  const int64_t nrows = (n - wave_base) < kPolWaveEnvs ? (n - wave_base) : kPolWaveEnvs;   // <= 0 for trailing waves of the last workgroup
  for (int q = threadIdx.x; q < total / 4; q += kPolBlock)
    *reinterpret_cast<float4*>(w + 4 * q) = *reinterpret_cast<const float4*>(W + 4 * q);
  stage_obs_rows(obs, wave_base, nrows, rows, lane);
  __syncthreads();   // the parameters are in LDS (the only workgroup barrier; every wave reaches it)
  if (nrows <= 0) return;
  float a[4];
  mlp_means<ACT>(w, H, rows, lane, a);
  if (CRITIC) {
    if (lane < nrows) out[wave_base + lane] = a[0];   // lanes 0..31: row 0 of the head tile of env l
  } else {
    actor_outputs(w + kMlpStd, lane, wave_base, nrows, deterministic, seed, counter, env_id_offset, a, arows, out, raw_actions, log_prob);
  }
}

}  // namespace rdv

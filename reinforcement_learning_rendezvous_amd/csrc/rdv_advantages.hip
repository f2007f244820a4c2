// rdv_advantages.hip — the GAE kernel of rdv_advantages.h and its launch, in a translation unit of its own (the objects of the other
// units do not change when it does).  The exported rdv_gae / rdv_rollout_advantages are in rdv_hip.hip, with the other entry points.
#include "rdv_advantages.h"

#pragma clang fp contract(off)   // no FMA anywhere in this unit: the recurrence is rounded operation by operation (rdv_advantages.h)

namespace rdv {

// One row of one env.  `A` and `nv` (values of row t + 1) are the carried chain; r / d / v are this row's loaded inputs.  Plain operators
// under the pragma above, one per rounding: HIP's __fmul_rn / __fadd_rn are inline functions of a header compiled with contraction on,
// and hipcc fused them into v_fmac_f32 here.
__device__ __forceinline__ void gae_row(float r, uint32_t d, float v, float g, float c, float& nv, float& A, float& ret) {
  const float nnt = 1.0f - (float)d;
  const float gnv = g * nv, bootstrap = gnv * nnt, target = r + bootstrap, delta = target - v;
  const float cn = c * nnt, carried = cn * A;
  A = delta + carried;
  ret = A + v;
  nv = v;
}

// A wave-uniform row offset, told to the compiler as such (scalar registers): the accesses below are `scalar row base + the lane's
// 32-bit offset`, so one vector register addresses every row.  Left to itself hipcc turns the row addresses into per-lane 64-bit
// induction variables, one per ring slot and array (132 vector registers at D = 8).
__device__ __forceinline__ int64_t row_base(int64_t k) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)k), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)k >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int D>
__global__ __launch_bounds__(kGaeBlock) void gae_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                                        const float* __restrict__ values, const float* __restrict__ last_value,
                                                        int32_t n_steps, int64_t n, float g, float c, float* __restrict__ advantages,
                                                        float* __restrict__ returns) {
  const int64_t base = (int64_t)blockIdx.x * kGaeBlock;
  const uint32_t lane = threadIdx.x;
  if (base + lane >= n) return;
  reward += base; done += base; values += base; advantages += base; returns += base;
  const int64_t ring = (int64_t)D * n;     // elements between a row and the row that takes its slot
  // the ring: slot j holds row t0 - j of the current group of D rows, then row t0 - j - D as soon as it has been consumed
  float r[D], v[D];
  uint32_t d[D];     // the done byte, zero-extended by its load (as bytes hipcc packs four slots into a register and waits for all of them)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const int32_t t = n_steps - 1 - j;
    const int64_t k = (int64_t)(t >= 0 ? t : 0) * n;    // (a group shorter than D: the slot is loaded and never used)
    r[j] = (reward + row_base(k))[lane]; d[j] = (done + row_base(k))[lane]; v[j] = (values + row_base(k))[lane];
  }
  float nv = (last_value + row_base(base))[lane], A = 0.0f;
  int32_t t0 = n_steps - 1;
  // whole groups with a whole group behind them: every slot is consumed and refilled, no row test
  for (; t0 >= 2 * D - 1; t0 -= D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int64_t k = (int64_t)(t0 - j) * n;
      const float rt = r[j], vt = v[j];
      const uint32_t dt = d[j];
      r[j] = (reward + row_base(k - ring))[lane]; d[j] = (done + row_base(k - ring))[lane]; v[j] = (values + row_base(k - ring))[lane];
      float ret;
      gae_row(rt, dt, vt, g, c, nv, A, ret);
      (advantages + row_base(k))[lane] = A; (returns + row_base(k))[lane] = ret;
    }
  }
  // the last one or two groups (wave-uniform tests: t is the same in every lane)
  for (; t0 >= 0; t0 -= D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int32_t t = t0 - j;
      if (t >= 0) {
        const int64_t k = (int64_t)t * n;
        const float rt = r[j], vt = v[j];
        const uint32_t dt = d[j];
        if (t >= D) { r[j] = (reward + row_base(k - ring))[lane]; d[j] = (done + row_base(k - ring))[lane]; v[j] = (values + row_base(k - ring))[lane]; }
        float ret;
        gae_row(rt, dt, vt, g, c, nv, A, ret);
        (advantages + row_base(k))[lane] = A; (returns + row_base(k))[lane] = ret;
      }
    }
  }
}

void gae_launch(const float* reward, const uint8_t* done, const float* values, const float* last_value, int32_t n_steps, int64_t n,
                float g, float c, float* advantages, float* returns, int depth, hipStream_t s) {
  const dim3 grid((unsigned)((n + kGaeBlock - 1) / kGaeBlock)), block(kGaeBlock);
#define RDV_GAE_LAUNCH(D) hipLaunchKernelGGL((gae_kernel<D>), grid, block, 0, s, reward, done, values, last_value, n_steps, n, g, c, advantages, returns)
  switch (depth ? depth : kGaeDepth) {
    case 2: RDV_GAE_LAUNCH(2); break;
    case 4: RDV_GAE_LAUNCH(4); break;
    case 16: RDV_GAE_LAUNCH(16); break;
    default: RDV_GAE_LAUNCH(8); break;
  }
#undef RDV_GAE_LAUNCH
}
static_assert(kGaeDepth == 8, "gae_launch's default case is kGaeDepth");

}  // namespace rdv

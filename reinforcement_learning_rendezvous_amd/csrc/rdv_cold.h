// rdv_cold.h — the kernels off the hot path: reset, state access / evaluator helpers, the evaluation summary.  One lane per env, launched
// by the C ABI (rdv_hip.hip).  Device code only.
#pragma once
#include "rdv_kernels.h"
#include "rdv_slots.h"

namespace rdv {

// reset() for all envs or where mask != 0; the env's prepared slot is refilled for the episode after the one that starts here
// (the bodies of the cold kernels are functions of the parameter block so that the kernels of parameter groups, csrc/rdv_groups.hip,
//  run the same code with their workgroup's own block)
template <typename ST>
__device__ __forceinline__ void reset_lane(const DevParams& P, const StepArgs& A, const uint8_t* mask, float* obs, int fresh) {
  using V = typename Vec4<ST>::type;
  const int64_t n = A.n;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  V* ws = reinterpret_cast<V*>(A.ws);
  if (mask && !mask[i]) return;
  Env e;
  load_env<ST>(ws, A.cs, i, e);
  if (fresh) e.episode = 0;   // first reset after create/seed: the workspace may hold anything
  const uint32_t counter = e.episode;
  reset_env<ST>(P, e, A.seed, A.env_id_offset + (uint64_t)i, tape_row_of(A.tape, A.tape_depth, n, i, counter));
  store_env<ST>(ws, A.cs, i, e, true);
  if (obs) {
    float o[RDV_OBS_DIM];
    observation(P, e, o);
    for (int j = 0; j < RDV_OBS_DIM; ++j) obs[i * RDV_OBS_DIM + j] = o[j];
  }
  refill_whole<ST>(A, P, i, counter + 1u);
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void reset_kernel(const DevParams* __restrict__ Pp, const StepArgs A, const uint8_t* mask, float* obs, int fresh) {
  reset_lane<ST>(*Pp, A, mask, obs, fresh);
}

enum { ACC_SET_STATE = 0, ACC_GET_STATE, ACC_GET_AUX, ACC_OBSERVE, ACC_DIAGNOSE, ACC_EVAL_BEGIN, ACC_CLEAR_HALTED };

// state access / evaluator helpers (cold paths; one lane per env, row-major host-facing arrays)
template <typename ST>
__device__ __forceinline__ void access_lane(const DevParams& P, void* ws_, int64_t n, int64_t cs, int what, const double* in, double* out, float* out_f32) {
  using V = typename Vec4<ST>::type;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  V* ws = reinterpret_cast<V*>(ws_);
  Env e;
  load_env<ST>(ws, cs, i, e);
  const ST tag = ST(0);
  if (what == ACC_SET_STATE) {          // monte_carlo.py:107-112: the 20 state reals only; flags and aux stay
    const double* s = in + i * RDV_STATE_DIM;
    for (int j = 0; j < 3; ++j) { e.rc[j] = canon(s[j], tag); e.vc[j] = canon(s[3 + j], tag); e.wc[j] = canon(s[10 + j], tag); e.wt[j] = canon(s[17 + j], tag); }
    for (int j = 0; j < 4; ++j) { e.qc[j] = canon(s[6 + j], tag); e.qt[j] = canon(s[13 + j], tag); }
    store_env<ST>(ws, cs, i, e, true);
  } else if (what == ACC_GET_STATE) {
    double* s = out + i * RDV_STATE_DIM;
    for (int j = 0; j < 3; ++j) { s[j] = e.rc[j]; s[3 + j] = e.vc[j]; s[10 + j] = e.wc[j]; s[17 + j] = e.wt[j]; }
    for (int j = 0; j < 4; ++j) { s[6 + j] = e.qc[j]; s[13 + j] = e.qt[j]; }
  } else if (what == ACC_GET_AUX) {
    double* s = out + i * 8;
    s[0] = rint((double)e.k * P.dt * 1e3) / 1e3; s[1] = e.bubble; s[2] = (e.flags & FLAG_COLLIDED) ? 1.0 : 0.0;
    s[3] = (double)(e.flags >> SUCCESS_SHIFT); s[4] = e.sum_dv; s[5] = e.sum_dw; s[6] = e.ep_ret; s[7] = (double)e.episode;
  } else if (what == ACC_OBSERVE) {
    float o[RDV_OBS_DIM];
    observation(P, e, o);
    for (int j = 0; j < RDV_OBS_DIM; ++j) out_f32[i * RDV_OBS_DIM + j] = o[j];
  } else if (what == ACC_DIAGNOSE) {
    Derived d;
    derive<false>(P, e, d);
    diagnostics(P, e, d, out + i * RDV_DIAG_DIM);
  } else if (what == ACC_CLEAR_HALTED) {   // rdv_restore into a RESET / CONTINUE handle: a halted flag of the snapshot is dropped
    e.flags &= ~FLAG_HALTED;
    store_env<ST>(ws, cs, i, e, true);
  } else {            // ACC_EVAL_BEGIN: the accumulators' k = 0 entries, from the state as it stands (after reset / set_state)
    Derived d;
    derive<false>(P, e, d);
    double dg[RDV_DIAG_DIM];
    diagnostics(P, e, d, dg);
    eval_accumulate(P, e, d, dg, 0.0, true, out + i * kEvalDim);
  }
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void access_kernel(const DevParams P, void* ws_, int64_t n, int64_t cs, int what, const double* in,
                                                        double* out, float* out_f32) {
  access_lane<ST>(P, ws_, n, cs, what, in, out, out_f32);
}

// The means CustomWandbCallback.evaluate_policy logs (custom_callbacks.py:254-298) over the batch's envs, from the evaluation
// accumulators and the final state: one wavefront reduction (DPP sums, fixed order) per 64 envs into that wave's 16-double slot; the
// host adds the slots in index order.
enum { EV_REW = 0, EV_LEN, EV_DIST, EV_DV, EV_DW, EV_SUCC, EV_COLLP, EV_TFIRST, EV_TFIRST_N, EV_MINPOS, EV_MINPOS_N, EV_AVGATT, EV_NCOLL, EV_NSUCC, EV_N, EV_SLOTS = 16 };
template <typename ST>
__device__ __forceinline__ void eval_summary_lane(const DevParams& P, const void* ws_, int64_t n, int64_t cs, const double* eval, double* partial) {
  using V = typename Vec4<ST>::type;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  double v[EV_N + 1];
#pragma unroll
  for (int j = 0; j <= EV_N; ++j) v[j] = 0.0;
  if (i < n) {
    Env e;
    load_env<ST>(reinterpret_cast<const V*>(ws_), cs, i, e);
    const double* acc = eval + i * kEvalDim;
    const double end_time = rint((double)e.k * P.dt * 1e3) / 1e3;      // :254
    const double steps = end_time / P.dt;                              // :255
    v[EV_REW] = acc[0]; v[EV_LEN] = end_time; v[EV_DIST] = sqrt(sumsq3(e.rc));                 // :258-260
    v[EV_DV] = e.sum_dv; v[EV_DW] = e.sum_dw; v[EV_SUCC] = (double)(e.flags >> SUCCESS_SHIFT);  // :261-263
    v[EV_COLLP] = acc[3] / steps * 100.0;                                                      // :264
    const bool has_t = acc[4] == acc[4], has_p = acc[5] == acc[5];
    v[EV_TFIRST] = has_t ? acc[4] : 0.0; v[EV_TFIRST_N] = has_t ? 1.0 : 0.0;                    // :265, nanmean :274-282
    v[EV_MINPOS] = has_p ? acc[5] : 0.0; v[EV_MINPOS_N] = has_p ? 1.0 : 0.0;                    // :266
    v[EV_AVGATT] = acc[2] / (steps + 1.0);                                                     // :267
    v[EV_NCOLL] = acc[3] > 0.0 ? 1.0 : 0.0; v[EV_NSUCC] = (e.flags >> SUCCESS_SHIFT) != 0u ? 1.0 : 0.0;   // :268-269
    v[EV_N] = 1.0;
  }
  double* slot = partial + (uint64_t)(i / kWave) * EV_SLOTS;
#pragma unroll
  for (int j = 0; j <= EV_N; ++j) {
    const double s = wave_sum_f64(v[j]);
    if (lane == 0 && (i - lane) < n) slot[j] = s;
  }
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void eval_summary_kernel(const DevParams P, const void* ws_, int64_t n, int64_t cs, const double* eval, double* partial) {
  eval_summary_lane<ST>(P, ws_, n, cs, eval, partial);
}

}  // namespace rdv

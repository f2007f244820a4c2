// rdv_policy_mlp.hip — the six instantiations of mlp_kernel (rdv_policy_mlp.h: tanh / ReLU / sigmoid x actor / critic) and their
// launches.  A translation unit of its own, as rdv_groups.hip is: the objects of rdv_hip.hip stay what they were.
#define RDV_POLICY_FUNCTIONS_ONLY
#include "rdv_policy_mlp.h"

namespace rdv {

template <bool CRITIC>
static const void* mlp_kernel_of(int activation) {
  switch (activation) {
    case RDV_ACT_RELU: return reinterpret_cast<const void*>(mlp_kernel<RDV_ACT_RELU, CRITIC>);
    case RDV_ACT_SIGMOID: return reinterpret_cast<const void*>(mlp_kernel<RDV_ACT_SIGMOID, CRITIC>);
    default: return reinterpret_cast<const void*>(mlp_kernel<RDV_ACT_TANH, CRITIC>);
  }
}

hipError_t mlp_raise_lds_limit() {
  for (int act = 0; act < 3; ++act) {
    hipError_t err = hipFuncSetAttribute(mlp_kernel_of<false>(act), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpMaxLdsBytes);
    if (err == hipSuccess) err = hipFuncSetAttribute(mlp_kernel_of<true>(act), hipFuncAttributeMaxDynamicSharedMemorySize, kMlpMaxLdsBytes);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

template <int ACT, bool CRITIC>
static void launch(const float* W, int block_floats, const float* obs, float* out, int64_t n, int deterministic, uint64_t seed,
                   uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  const dim3 grid((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs));
  hipLaunchKernelGGL((mlp_kernel<ACT, CRITIC>), grid, dim3(kPolBlock), mlp_lds_bytes(block_floats), s, W, obs, out, n, deterministic, seed,
                     counter, env_id_offset, raw_actions, log_prob);
}

void mlp_launch_act(int activation, const float* W, int block_floats, const float* obs, float* actions, int64_t n, int deterministic,
                    uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  switch (activation) {
    case RDV_ACT_RELU: launch<RDV_ACT_RELU, false>(W, block_floats, obs, actions, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
    case RDV_ACT_SIGMOID: launch<RDV_ACT_SIGMOID, false>(W, block_floats, obs, actions, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
    default: launch<RDV_ACT_TANH, false>(W, block_floats, obs, actions, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s); break;
  }
}

void mlp_launch_value(int activation, const float* W, int block_floats, const float* obs, float* values, int64_t n, hipStream_t s) {
  switch (activation) {
    case RDV_ACT_RELU: launch<RDV_ACT_RELU, true>(W, block_floats, obs, values, n, 1, 0, 0, 0, nullptr, nullptr, s); break;
    case RDV_ACT_SIGMOID: launch<RDV_ACT_SIGMOID, true>(W, block_floats, obs, values, n, 1, 0, 0, 0, nullptr, nullptr, s); break;
    default: launch<RDV_ACT_TANH, true>(W, block_floats, obs, values, n, 1, 0, 0, 0, nullptr, nullptr, s); break;
  }
}

}  // namespace rdv

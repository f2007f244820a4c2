// rdv_policy_lstm.hip — the kernels of the recurrent policy (rdv_policy_lstm.h: the cell for H = 32 / 64 / 128 / 256, the trunk for
// tanh / ReLU / sigmoid x actor / critic, each also in its set form, and the state reset) and their launches.  A translation unit of
// its own, as rdv_policy_mlp.hip is: the objects of the other units stay what they were.
#define RDV_POLICY_FUNCTIONS_ONLY
#define RDV_LSTM_KERNELS
#include "rdv_policy_lstm.h"

namespace rdv {

static inline dim3 lstm_grid(int64_t n) { return dim3((unsigned)((n + kPolBlockEnvs - 1) / kPolBlockEnvs)); }

template <int H>
static void launch_cell(const float* W, int block_floats, const int32_t* tile_member, const float* obs, const uint8_t* start, const float* h,
                        const float* c, float* h_next, float* c_out, int64_t n, hipStream_t s) {
  if (tile_member)
    hipLaunchKernelGGL((lstm_cell_kernel<H, LstmSetBlocks>), lstm_grid(n), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, n,
                       LstmSetBlocks{tile_member, block_floats});
  else hipLaunchKernelGGL(lstm_cell_kernel<H>, lstm_grid(n), dim3(kPolBlock), 0, s, W, obs, start, h, c, h_next, c_out, n);
}

void lstm_launch_cell(int H, const float* W, int block_floats, const int32_t* tile_member, const float* obs, const uint8_t* start, const float* h,
                      const float* c, float* h_next, float* c_out, int64_t n, hipStream_t s) {
  switch (H) {
    case 32: launch_cell<32>(W, block_floats, tile_member, obs, start, h, c, h_next, c_out, n, s); break;
    case 64: launch_cell<64>(W, block_floats, tile_member, obs, start, h, c, h_next, c_out, n, s); break;
    case 128: launch_cell<128>(W, block_floats, tile_member, obs, start, h, c, h_next, c_out, n, s); break;
    default: launch_cell<256>(W, block_floats, tile_member, obs, start, h, c, h_next, c_out, n, s); break;
  }
}

template <int ACT, bool CRITIC>
static void launch_trunk(const float* W, int block_floats, const int32_t* tile_member, const float* h_next, float* h_commit, float* out, int64_t n,
                         int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions, float* log_prob, hipStream_t s) {
  if (tile_member)
    hipLaunchKernelGGL((lstm_trunk_kernel<ACT, CRITIC, LstmSetBlocks>), lstm_grid(n), dim3(kPolBlock), 0, s, W, h_next, h_commit, out, n, deterministic,
                       seed, counter, env_id_offset, raw_actions, log_prob, LstmSetBlocks{tile_member, block_floats});
  else
    hipLaunchKernelGGL((lstm_trunk_kernel<ACT, CRITIC>), lstm_grid(n), dim3(kPolBlock), 0, s, W, h_next, h_commit, out, n, deterministic, seed,
                       counter, env_id_offset, raw_actions, log_prob);
}

void lstm_launch_trunk(int activation, bool critic, const float* W, int block_floats, const int32_t* tile_member, const float* h_next, float* h_commit,
                       float* out, int64_t n, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset, float* raw_actions,
                       float* log_prob, hipStream_t s) {
#define RDV_LSTM_TRUNK(ACT)                                                                                                               \
  if (critic) launch_trunk<ACT, true>(W, block_floats, tile_member, h_next, h_commit, out, n, 1, 0, 0, 0, nullptr, nullptr, s);           \
  else launch_trunk<ACT, false>(W, block_floats, tile_member, h_next, h_commit, out, n, deterministic, seed, counter, env_id_offset, raw_actions, log_prob, s)
  switch (activation) {
    case RDV_ACT_RELU: RDV_LSTM_TRUNK(RDV_ACT_RELU); break;
    case RDV_ACT_SIGMOID: RDV_LSTM_TRUNK(RDV_ACT_SIGMOID); break;
    default: RDV_LSTM_TRUNK(RDV_ACT_TANH); break;
  }
#undef RDV_LSTM_TRUNK
}

void lstm_launch_reset(float* h, float* c, const uint8_t* mask, int64_t n, int H, hipStream_t s) {
  const int64_t quads = n * (H / 4);
  hipLaunchKernelGGL(lstm_reset_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, h, c, mask, n, H);
}

}  // namespace rdv

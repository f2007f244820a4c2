// rdv_policy_sets.h — policy sets: P member networks of ONE architecture, each owning a contiguous range of a batch's rows, evaluated
// by one launch (include/rdv.h, "Policy sets").  The kernels of rdv_policy.h / rdv_policy_mlp.h give each workgroup 256 consecutive rows
// and stage ONE parameter block into LDS behind their only barrier; the set forms (rdv_policy_sets.hip) stage
// W + tile_member[blockIdx.x] * block_floats instead of W — one more wave-uniform scalar load per workgroup, nothing else — and then run
// the same device functions (stage_obs_rows, actor_means, actor_outputs, mlp_means).  Every range but the last is a multiple of 256 rows
// (the rule of parameter groups, rdv_param_groups_check), so a workgroup never spans two members.
//
// Memory of a set handle, one allocation: [P blocks of block_floats floats][tile table: one int32 member index per 256-row tile].
// The blocks hold exactly the bytes pack_policy_weights / pack_mlp_weights give for stand-alone handles.
//
// The critic runs over [k, n] rows (a rollout's obs is [T, N, 17]) and membership follows the ENV index, so the value kernels take a
// second grid dimension: tile x of row block y reads rows y * n + x * 256 ..., and the same tile table serves every y.  ALIGNMENT: the
// full-wave path of stage_obs_rows loads 16 bytes per lane from obs + row * 17; a row is 68 bytes, so y * n rows are a multiple of
// 16 bytes only when y * n is a multiple of 4.  The set kernels take that path only when the wave's source address is 16-byte aligned
// and the element path otherwise (the same values: both are plain copies into the wave's LDS rows).
//
// This header holds declarations only; rdv_hip.hip includes it and its objects stay what they were.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdv {

constexpr int kSetTile = 256;                 // rows per workgroup = kPolBlockEnvs = kGroupTile
constexpr int64_t kSetMaxRowBlocks = 65535;   // gridDim.y's limit: more row blocks than this go out as several launches

// hipFuncAttributeMaxDynamicSharedMemorySize of the set kernels (shipped: the two of the 17-64-64 tanh block; otherwise the six mlp ones)
hipError_t sets_raise_lds_limit(bool shipped_arch);
// One launch for `rows` rows (the set's row count); `tile_member`: device, one entry per 256-row tile.
void sets_launch_act(bool shipped_arch, int activation, const float* W, int block_floats, const int32_t* tile_member, const float* obs,
                     float* actions, int64_t rows, int deterministic, uint64_t seed, uint64_t counter, uint64_t env_id_offset,
                     float* raw_actions, float* log_prob, hipStream_t s);
// `row_blocks` blocks of `rows` rows each (obs [row_blocks, rows, 17], values [row_blocks, rows]): one launch per 65,535 row blocks
void sets_launch_value(bool shipped_arch, int activation, const float* W, int block_floats, const int32_t* tile_member, const float* obs,
                       float* values, int64_t rows, int64_t row_blocks, hipStream_t s);

}  // namespace rdv

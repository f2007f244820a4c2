// rdv_groups.hip — the kernels of parameter groups (rdv_set_param_groups, include/rdv.h): one batch, G contiguous groups of envs, each
// with its own DevParams block, ONE launch.  The parameter block is wave-uniform by design (every field a scalar load) and a workgroup
// owns 256 consecutive envs in every step layout, so groups that begin on 256-env boundaries cost one more scalar load per workgroup:
// the group index of the workgroup's tile, read from a table in device memory with the LOGICAL block index (behind the XCD reorder),
// and then P = Pp[group] instead of P = *Pp.  A group may not begin inside a tile because the reset-by-part phase shares one block
// among the four waves of a workgroup (refill_pass_lds).
// There is no step kernel body here: the grouped step kernels are instantiations of step_kernel_parts (rdv_step.h) and step_kernel
// (rdv_fused.h) with the tile table as one more argument, and the cold kernels call the lane functions of rdv_cold.h — the same code on
// the same inputs, so an env's results are bit for bit those of a stand-alone handle created with its group's parameters
// (tests/test_gpu_param_groups.py).  What is here: group_block, the cold grouped kernels and the launches.  A translation unit of its
// own, with the flags of rdv_hip.hip, so that that file's objects do not change when a grouped instantiation is added.
#include "rdv_kernels.h"
#include "rdv_slots.h"
#include "rdv_fused.h"
#include "rdv_step.h"
#include "rdv_cold.h"
#include "rdv_launch.h"
#include "rdv_groups.h"

namespace rdv {

// The group of a workgroup's tile.  `lblock` is computed from blockIdx and a kernel argument, so the index, the table entry and
// with them the address of every parameter field are wave-uniform: the table entry is ONE scalar load, requested at kernel entry (it
// needs nothing but the block index) and waited for where the first parameter is used, behind the requests of the state.
// (The step kernels call it from their grouped instantiations only: a dependent call, looked up where they are instantiated — here.)
__device__ __forceinline__ const DevParams& group_block(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, int64_t lblock) {
  const int g = __builtin_amdgcn_readfirstlane(tile_group[lblock]);
  return Pp[g];
}

// ---------------------------------------------------------------------------------------------------------------
// The cold kernels: one lane per env, 256-thread workgroups in env order, so blockIdx.x is the tile (rdv_cold.h has the bodies).
template <typename ST>
__global__ __launch_bounds__(kBlock) void reset_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, const StepArgs A,
                                                              const uint8_t* mask, float* obs, int fresh) {
  reset_lane<ST>(group_block(Pp, tile_group, blockIdx.x), A, mask, obs, fresh);
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void access_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, void* ws_, int64_t n,
                                                               int64_t cs, int what, const double* in, double* out, float* out_f32) {
  access_lane<ST>(group_block(Pp, tile_group, blockIdx.x), ws_, n, cs, what, in, out, out_f32);
}
template <typename ST>
__global__ __launch_bounds__(kBlock) void eval_summary_kernel_groups(const DevParams* __restrict__ Pp, const int32_t* __restrict__ tile_group, const void* ws_,
                                                                     int64_t n, int64_t cs, const double* eval, double* partial) {
  eval_summary_lane<ST>(group_block(Pp, tile_group, blockIdx.x), ws_, n, cs, eval, partial);
}

// ---------------------------------------------------------------------------------------------------------------
static_assert(kBlock == kGroupTile, "one workgroup of a step kernel = one tile of the group table = one reset-by-part pass");
using TileTable = const int32_t* __restrict__;   // top-level and __restrict__, like the parameter pointer: the entry and every field stay scalar loads
// The grouped step kernels by the names rdv_debug_last_kernel reports: the shared templates with the table's type, nothing of their own
template <typename ST, bool kAll> constexpr auto step_kernel_groups = &step_kernel_parts<ST, kAll, TileTable>;
template <typename ST, bool kDiag, bool kRaw> constexpr auto step_kernel_groups_lane = &step_kernel<ST, kDiag, false, kRaw, TileTable>;
#define RDV_K_PARTS(ST, B) step_kernel_groups<ST, B>
#define RDV_K_DIAG(ST, B) step_kernel_groups_lane<ST, true, B>
const char* launch_step_groups(bool f32, bool all, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A) {
  const char* name;
  RDV_LAUNCH_BY(name, f32, all, RDV_K_PARTS, grid, dim3(kBlock), s, RDV_HOT_ARGS(A, T.params), T.tile_group, A);
  return name;
}
const char* launch_step_groups_lane(bool f32, bool diag, bool raw, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A) {
  const char* name;
  if (diag) RDV_LAUNCH_BY(name, f32, raw, RDV_K_DIAG, grid, dim3(kBlock), s, RDV_HOT_ARGS(A, T.params), T.tile_group, A);
  else if (f32) RDV_LAUNCH(name, (step_kernel_groups_lane<float, false, true>), grid, dim3(kBlock), s, RDV_HOT_ARGS(A, T.params), T.tile_group, A);
  else RDV_LAUNCH(name, (step_kernel_groups_lane<double, false, true>), grid, dim3(kBlock), s, RDV_HOT_ARGS(A, T.params), T.tile_group, A);   // (raw: the callers' only other case)
  return name;
}
#undef RDV_K_DIAG
#undef RDV_K_PARTS
void launch_reset_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A, const uint8_t* mask, float* obs, int fresh) {
  if (f32) hipLaunchKernelGGL(reset_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, A, mask, obs, fresh);
  else hipLaunchKernelGGL(reset_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, A, mask, obs, fresh);
}
void launch_access_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, void* ws, int64_t n, int64_t cs, int what, const double* in, double* out,
                          float* out_f32) {
  if (f32) hipLaunchKernelGGL(access_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, what, in, out, out_f32);
  else hipLaunchKernelGGL(access_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, what, in, out, out_f32);
}
void launch_eval_summary_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const void* ws, int64_t n, int64_t cs, const double* eval, double* partial) {
  if (f32) hipLaunchKernelGGL(eval_summary_kernel_groups<float>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, eval, partial);
  else hipLaunchKernelGGL(eval_summary_kernel_groups<double>, grid, dim3(kBlock), 0, s, T.params, T.tile_group, ws, n, cs, eval, partial);
}

}  // namespace rdv

// rdv_groups.h — host entries of the kernels of parameter groups (csrc/rdv_groups.hip): a batch divided into contiguous groups of envs
// that begin on 256-env boundaries, each with its own DevParams block (rdv_set_param_groups, include/rdv.h).
#pragma once
#include "rdv_kernels.h"
namespace rdv {
constexpr int kGroupTile = kBlock;   // a tile of the table = the 256 envs of one workgroup in every grouped kernel
// What a grouped kernel reads instead of the handle's one block: G blocks, and the group of every 256-env tile.  The table has an entry
// for every LOGICAL workgroup a launch can have — the tiles of the batch rounded up to a multiple of 8, because the XCD order pads the
// grid (rdv_kernels.h: xcd_order_by_size); the padding entries repeat the last group.
struct GroupTable {
  const DevParams* params;     // [G], device
  const int32_t* tile_group;   // [tiles rounded up to 8], device
};
// step_kernel_groups<ST, all> = step_kernel_parts<ST, all, TileTable> (rdv_step.h): the reset-by-part kernel with the workgroup's own block (`grid`, A.xcd_per, A.stagger,
// A.stream_rows as rdv_step sets them for step_kernel_parts).  Returns the name of the kernel it launched.
const char* launch_step_groups(bool f32, bool all, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A);
// step_kernel_groups_lane<ST, diag, raw> = step_kernel<ST, diag, false, raw, TileTable> (rdv_fused.h): the in-lane kernel (evaluator build, first step after rdv_set_state) likewise
const char* launch_step_groups_lane(bool f32, bool diag, bool raw, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A);
// reset_kernel / access_kernel / eval_summary_kernel with the workgroup's own block (arguments as in rdv_cold.h)
void launch_reset_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const StepArgs& A, const uint8_t* mask, float* obs, int fresh);
void launch_access_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, void* ws, int64_t n, int64_t cs, int what, const double* in, double* out,
                          float* out_f32);
void launch_eval_summary_groups(bool f32, dim3 grid, hipStream_t s, const GroupTable& T, const void* ws, int64_t n, int64_t cs, const double* eval, double* partial);
}  // namespace rdv

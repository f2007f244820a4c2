// rdv_launch.h — how the host launches a one-launch step kernel, for the translation units that do (rdv_hip.hip, rdv_general.hip,
// rdv_groups.hip): the seven hot arguments in front of the StepArgs (rdv_kernels.h: hot_args), and the kernel's name as it is spelled at
// the launch, which is what rdv_debug_last_kernel returns.  Host code only.
#pragma once
#include "rdv_kernels.h"

// The arguments of a step kernel are RDV_HOT_ARGS(A, params), A — a grouped instantiation (rdv_step.h: step_kernel_parts) has its tile
// table between the two.
#define RDV_HOT_ARGS(A, PARAMS) (A).ws, (A).actions, PARAMS, (A).n, (A).stats, (A).obs, (A).reward
// RDV_LAUNCH(name, (kernel<...>), grid, block, stream, arguments...): the launch, and `name` = "kernel<...>".  The kernel stands in
// parentheses because its template arguments hold commas.
#define RDV_NAME_OF(...) #__VA_ARGS__
#define RDV_LAUNCH(NAME, KERNEL, GRID, BLOCK, STREAM, ...) do { hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, STREAM, __VA_ARGS__); NAME = RDV_NAME_OF KERNEL; } while (0)
// One of the four instantiations K(float | double, true | false) of a kernel, by the storage type and FLAG; K is a macro of two
// arguments that spells the instantiation.
#define RDV_LAUNCH_BY(NAME, F32, FLAG, K, ...) do {                                                                                \
    if (F32) { if (FLAG) RDV_LAUNCH(NAME, (K(float, true)), __VA_ARGS__); else RDV_LAUNCH(NAME, (K(float, false)), __VA_ARGS__); }  \
    else { if (FLAG) RDV_LAUNCH(NAME, (K(double, true)), __VA_ARGS__); else RDV_LAUNCH(NAME, (K(double, false)), __VA_ARGS__); } } while (0)

// rdv_advantages.h — generalised advantage estimation over the rows of a rollout (rdv_gae, include/rdv.h): SB3's
// RolloutBuffer.compute_returns_and_advantage as ONE kernel for all T steps, bit for bit what that loop gives in NumPy float32.
//
// The recurrence, for t = T-1 .. 0 and each env, every operation rounded to fp32 on its own, in this association:
//     nnt   = 1 - (float)done[t]
//     nv    = t == T-1 ? last_value : values[t+1]
//     delta = ((reward[t] + (g * nv) * nnt) - values[t])           g = (float)gamma
//     A     = delta + ((c * nnt) * A)                               c = (float)(gamma * gae_lambda), A = 0 before the first step
//     advantages[t] = A,  returns[t] = A + values[t]
// hipcc contracts a * b + c into an FMA on the device by default, which rounds once where NumPy rounds twice and changes the last bit:
// the translation unit switches contraction off (#pragma clang fp contract(off)) and writes the chain in plain operators, one per
// rounding.  (HIP's __fmul_rn / __fadd_rn do NOT prevent it: they are inline functions of a header compiled with contraction on, and
// hipcc fused them into v_fmac_f32.)  The gfx950 assembly of the unit holds no v_fma / v_fmac / v_mad on floats.
//
// Layout.  One env per lane: row t of a [T,N] array is N consecutive floats (bytes for `done`), so every access of a wave is one
// contiguous segment.  t runs backwards in a loop; the chain of A is sequential and cannot be split over T without changing the
// rounding (segments + a carry fix-up re-associate the products), so a lane walks all T rows of its env.  What does not depend on
// the chain are the ADDRESSES: the loads of the kGaeDepth rows in front of the ones in use are in flight in a register ring (three
// registers per row: reward, done, values); a slot is refilled with the row kGaeDepth earlier when its row is consumed.  As hipcc
// schedules it, the refills of a group of kGaeDepth rows are issued together at the head of the group and waited for at the head of the
// next: kGaeDepth rows in flight per round trip while kGaeDepth rows are computed and stored.  values[t+1] is the previous row's
// values[t] and is kept, not loaded again.  64-bit index arithmetic throughout (T x N passes 2^31 at 512 x 4.2 M); the row part of an
// address is wave-uniform and held in scalar registers.  One wave per workgroup, so that a small batch spreads over as many CUs as it
// has waves: at small N the kernel is bound by the latency of T / kGaeDepth round trips per wave, not by bandwidth (DESIGN.md
// section 5 has the figures).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rdv {

constexpr int kGaeBlock = 64;    // one wave per workgroup
constexpr int kGaeDepth = 8;     // rows in flight per lane; by measurement (tools/gae_time.py): the fastest of 2 / 4 / 8 / 16 at 512 x 4,096, within 3 % of
                                 // the fastest (4) at 64 x 65,536 and 64 x 524,288

// The launch (rdv_advantages.hip).  `depth`: 0 = kGaeDepth; 2, 4, 8 or 16 = that instantiation (tools/gae_time.py times them side by
// side; results do not depend on it).  The caller has checked the arguments.
void gae_launch(const float* reward, const uint8_t* done, const float* values, const float* last_value, int32_t n_steps, int64_t n,
                float g, float c, float* advantages, float* returns, int depth, hipStream_t s);

}  // namespace rdv

// rdv_step.h — the one-launch step kernels that share the work of a reset inside the workgroup: step_kernel_parts (batches beyond one
// workgroup per CU: the reset by part) and step_kernel_split (smaller batches: step waves beside service waves), and prepare_kernel,
// which re-derives the slots of the persistent kernels after them.  Launched by rdv_step (rdv_hip.hip).  Device code only.
#pragma once
#include "rdv_kernels.h"
#include "rdv_slots.h"

namespace rdv {

// Slots of all envs, re-derived from the envs' current episode indices: run before a persistent kernel (rdv_step_many, rdv_rollout)
// whenever something outside them changed what a reset returns (parameters, tape, seed, restore) or advanced episodes without
// them (rdv_step: its kernels compute resets in registers and do not touch the slots).
template <typename ST>
__global__ __launch_bounds__(kBlock) void prepare_kernel(const DevParams* __restrict__ Pp, const StepArgs A) {
  using V = typename Vec4<ST>::type;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const V c5 = reinterpret_cast<const V*>(A.ws)[5 * A.cs + i];
  refill_whole<ST>(A, *Pp, i, s2u(c5.w));
}

// ---------------------------------------------------------------------------------------------------------------
// Fused variant with the reset shared BY PART inside the workgroup (training build: no diagnostics, reference bodies, normalised
// state).  Everything up to the reset is step_kernel; a lane whose episode ended lists its env in LDS instead of resetting it, and
// after a workgroup barrier the four waves write the resets of the listed envs (~13 of 256 with random actions) together — wave w
// does part w (rc+vc+bookkeeping | qc+wc | qt | wt: reset_fields<ST, kPart>) for all of them, ~13 active lanes, straight into the
// envs' state chunks in HBM and their observation rows in LDS (LiveStore) — then a second barrier and the coalesced row stores.
// The in-lane form runs the whole ~900-instruction reset with ~3 active lanes in 96 % of the waves: about half of that kernel's
// vector instructions (SQ_INSTS_VALU 1,645 per wave, profiles/r02_sq_counters_4M.csv), and at three waves per SIMD they are not
// hidden.  Here every wave issues one part (~150-350 instructions) and the four stay balanced — unlike the variant that left the
// whole resets to the workgroup's last wave (profiles/r02_n_sweep_compacted_reset.csv), which held a wave slot and the LDS for a
// lone serial chain.  Same expressions on the same inputs: bit-identical results.  (Forced to 128 VGPRs for four waves per SIMD it
// spills 16 dwords and loses: 342 against 315 us at 4.2 M envs.)
// Parameter groups (rdv_groups.hip) instantiate this kernel with G = the pointer to the tile table, `const int32_t* __restrict__`, named
// explicitly: the table is then one more top-level argument and the workgroup runs with the block of its tile's group (group_block, there)
// instead of the handle's one block.  That is the only difference, so a grouped env's results are those of a stand-alone handle by
// construction.  Without G the argument does not exist and the kernel is what it was before there were groups.
template <typename ST, bool kAll, typename... G>   // kAll: on_done != HALT — every lane runs the transition (advance_all)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(sizeof(ST) == 4 ? RDV_PARTS_WAVES : 3))) void step_kernel_parts(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                             uint64_t* stats_hot, float* obs_hot, float* reward_hot, G... tile_group, const StepArgs A_rest) {
  static_assert(sizeof...(G) <= 1, "G is empty or the type of the tile table");
  const StepArgs A = hot_args(A_rest, ws_hot, actions_hot, n_hot, stats_hot, obs_hot, reward_hot);
  using V = typename Vec4<ST>::type;
  __shared__ __attribute__((aligned(16))) float lds[kBlock * RDV_OBS_DIM];   // observation rows [256][17]; before that, per wave, the action rows
  __shared__ uint32_t job_kind[kBlock];
  __shared__ uint32_t job_counter[kBlock];
  __shared__ uint16_t lists[kGroupWaves * kBlock];
  static_assert(kBlock == kGroupEnvs, "refill_pass_lds is written for 256-env workgroups");
  const DevParams* Pb = Pp;   // the handle's one block
  const int lane = threadIdx.x & (kWave - 1);
  // Everything that is the same for the 64 lanes of a wave is computed on the scalar unit (readfirstlane tells the compiler that the wave
  // index is uniform): the wave's first env, its row count, the bases of its slices of every array.  A lane then addresses memory as
  // [uniform base in SGPRs] + [32-bit lane offset] — as 64-bit per-lane indices these held ~10 vector registers for the whole kernel.
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8); with A.xcd_per != 0 XCD x walks its own
  // contiguous eighth of the envs in ascending order instead of every 8th workgroup of the whole batch (see kXcdOrderMaxEnvs)
  const int64_t lblock = A.xcd_per ? (int64_t)(blockIdx.x & 7) * A.xcd_per + (blockIdx.x >> 3) : (int64_t)blockIdx.x;
  if constexpr (sizeof...(G) != 0) Pb = &group_block(Pp, tile_group..., lblock);   // the LOGICAL block: the table is in env order
  const DevParams& P = *Pb;   // (the four waves of the reset by part share it: a group begins on a tile boundary)
  const int64_t block_base = lblock * kBlock;
  const int64_t wave_base = block_base + wave_in_block * kWave;
  const int64_t n = A.n;
  const int64_t rows = (n - wave_base) < kWave ? (n - wave_base) : kWave;    // valid envs of this wave (may be <= 0)
  const bool active = lane < rows;
  float* wl = lds + wave_in_block * (kWave * RDV_OBS_DIM);
  V* ws = reinterpret_cast<V*>(A.ws);
  const bool resets = A.on_done == RDV_ON_DONE_RESET;   // kernel-uniform: the barriers below are executed by all waves or by none
  RDV_STAMP_DECL
  RDV_STAMP(0);
  // Staggered start (round 4): a launch of a few rounds of workgroups runs in lockstep — every resident wave loads at once (a 35 MB
  // burst), then all compute, then the next round loads at once — so the memory system idles while the SIMDs work and vice versa.
  // The first-round workgroups (the first 4 per CU) therefore start `stagger` x 512 cycles apart by their slot on the CU; their
  // successors inherit the phase.  Pure delay, no effect on results; sized by kStagger* below (profiles/r04_stagger.txt).
  if (A.stagger && blockIdx.x < 1024u) {
    const int slot = (int)(blockIdx.x >> 8);             // the k-th workgroup of its CU (256 CUs, dealt round-robin)
    for (int k = 0; k < slot * A.stagger; ++k) __builtin_amdgcn_s_sleep(8);   // 512 cycles each
  }

  {
    V* wsw = ws + wave_base;                             // this wave's slice of every chunk array: chunk c of lane l at wsw[c * cs + l]
    const StepArgs Aw = wave_outputs(A, wave_base);      // ... and of the per-env outputs
    Env e;
    uint64_t* slot = A.stats + (uint64_t)(wave_base / kWave) * kStatWords;
    uint64_t slot_pre;
    float a[RDV_ACT_DIM];
    constexpr bool kPinned = kAll && sizeof(ST) == 4;
    PinnedInputs pin;
    if constexpr (kPinned) {
      pinned_state(A, wave_base, lane, pin, e);          // state chunks, action row, statistics slot: all requested together (rdv_kernels.h: PinnedInputs)
    } else if constexpr (kAll) {
      TileInputs<ST> in;
      tile_fetch<ST>(A, wave_base, lane, in);
      unpack_env<ST>(in.c, e);
      slot_pre = in.slot_pre;
#pragma unroll
      for (int k = 0; k < 3; ++k) { a[2 * k] = in.a[k].x; a[2 * k + 1] = in.a[k].y; }
    } else {
      if (active) load_env<ST>(wsw, A.cs, lane, e);
      slot_pre = rows > 0 ? stats_preload(slot, lane) : 0ull;   // (a padding workgroup of the XCD order has no envs)
      load_actions(A.actions + wave_base * RDV_ACT_DIM, 0, lane, active, a);
    }
    RDV_STAMP_STATE(e);
    RDV_STAMP(1);
    StepResult r;
    const RowSink my_row{wl + lane * RDV_OBS_DIM};      // the observation is staged as it is formed
    constexpr bool kPack = sizeof(ST) == 4;   // (see step_kernel_split)
    V packed[kChunks];
    bool stepped;
    auto actions_ready = [&](double& after) { if constexpr (kPinned) pinned_rest(pin, after, a, slot_pre); };
    if constexpr (kAll) { advance_all<ST>(P, e, a, r, my_row, kPack ? packed : nullptr, actions_ready); stepped = active; }
    else stepped = advance<ST, false, false, false>(A, P, wave_base + lane, active, e, a, r, my_row, NoHook(), kPack ? packed : nullptr);
    RDV_STAMP(2);
    const bool fin = stepped && r.done;
    stats_update(slot, slot_pre, lane, stepped, fin, r.reason, e.flags, e.k, e.ep_ret, e.sum_dv, e.sum_dw);
    store_step_outputs<true>(Aw, lane, active, fin, r, e, my_row.row);
    const bool to_reset = fin && resets;
    halt_if_done<ST>(A, fin, e, kPack ? packed : nullptr);
    if (resets) {
      job_kind[threadIdx.x] = to_reset ? JOB_REFILL : JOB_NONE;
      job_counter[threadIdx.x] = e.episode;
    }
    if (stepped && !to_reset) { if (kPack) store_chunks<ST>(wsw, A.cs, lane, packed, false); else store_env<ST>(wsw, A.cs, lane, e, false); }   // a listed env's state is written by the parts, all seven chunks
  }
  RDV_STAMP(3);
  if (resets) {
    __syncthreads();   // the workgroup's finished envs are listed, every observation row is staged
    RDV_STAMP(4);
    LiveStore<ST> L;
    L.ws = ws; L.rows = lds; L.cs = A.cs; L.base = block_base;
    refill_pass_lds<ST>(wave_in_block, lane, P, L, job_kind, job_counter, lists + wave_in_block * kBlock, block_base, n, A.seed,
                        A.env_id_offset, A.tape, A.tape_depth);
    RDV_STAMP(5);
    __syncthreads();   // SB3 DummyVecEnv semantics: the rows of the listed envs now hold the first observation of the next episode
  } else {
    wave_lds_fence();
  }
  RDV_STAMP(6);
  if (A.stream_rows) store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);   // kernel-uniform: see StepArgs::stream_rows
  else store_obs_rows<false>(A.obs, wave_base, rows, lane, wl);
  RDV_STAMP(7);
  RDV_STAMP_FLUSH((uint64_t)blockIdx.x * (kBlock / kWave) + wave_in_block)
}

// ---------------------------------------------------------------------------------------------------------------
// Split-role variant for a chip that is NOT full (N <= ~98k envs: one transition wave per SIMD): a 512-thread workgroup owns 256
// envs.  Waves 0-3 ("step waves") do the whole transition for their 64 envs exactly as the fused kernel does, except the in-lane
// reset.  Waves 4-7 ("service waves") run beside them — an 8-wave workgroup places waves w and w+4 on the same SIMD, so every SIMD
// holds one of each — and compute every env's NEXT initial state IN REGISTERS while the step runs (it depends only on seed, env id
// and episode index).  After the single workgroup barrier a service lane whose env finished forms the observation of that state and
// writes both straight to HBM; the step waves have nothing left to do.  Same arithmetic, same results as the fused variant.
// The next-state work is done for every env and used by ~5 %.  Round 2 built the alternative the first review asked for — the next
// state persisted in HBM per env (rdv_slots.h), copied where an episode ends and refilled once per episode by compacted passes —
// for this kernel and for the fused one, and measured it (profiles/r02_*): 8.2 us per launch against 7.3 for this form at 65,536
// envs, 437 us against 317 at 4 M envs.  At one wave per SIMD the launch is a latency chain (1.2 us until the inputs are in, 1.9 us of
// transition, ~1 us of outputs, ~1.6 us of launch boundary: tools/ubench_stream.hip measures 4.0 us for the bare stream and
// boundary); the service waves' arithmetic runs in issue slots that are idle anyway and their results are in registers at the
// barrier, whereas a slot has to be fetched (a dependent, sparse access) exactly on that chain.  When the chip is full the step is
// bound by memory latency and request rate (59 % of the wave-cycles parked on s_waitcnt, profiles/r02_sq_counters_4M.csv), and
// slots add ~600 B of sparse traffic per reset where the in-lane reset adds none.  The slots stay where they do pay: in LDS, inside
// the persistent kernels (rdv_step_many.h, rdv_rollout.h).  (Also measured: the service waves idle until the barrier and then write
// the resets of the finished envs only, by part, as step_kernel_parts does, while the step waves do statistics and outputs — no
// speculative work at all: 8.2 us against 7.8 at 65,536 envs, 6.7 against 5.8 at 16,384.  The part is serial work after the barrier;
// the speculative reset costs nothing on the chain.  Wave priorities — s_setprio on the step waves, or on the service waves — change
// nothing either: 7.81-7.85 us in every combination.)
// The observation rows leave this kernel with non-temporal stores (store_obs_rows<true>): measured with tools/lib_ab.py, same box,
// alternating child processes — 7.54 -> 7.13 us per launch at 65,536 envs, 6.24 -> 6.08 at 32,768; non-temporal LOADS of the actions
// cost 0.4 us, non-temporal stores of reward / done / reason or of the state change nothing, and at 524,288 envs (fused kernel) streaming rows lose
// 1 %.  With the actor kernel reading the rows in the next launch (rdv_policy_act + rdv_step per step) the pair is unchanged, 15.8 us.
constexpr int kSplitEnvs = 256;      // envs per workgroup
constexpr int kSplitBlock = 512;     // 8 waves

// The refill workgroup of step_kernel_split's slot form, waves 0-3: the envs [base, base + 256) whose episode has just begun (k == 0) and
// whose slot does not hold the reset that ends it (tag != episode + 1) get that reset into their slot.  Wave w reads k, episode and tag
// of envs 64 w + lane and posts them in LDS; behind the workgroup's own barrier all four compact the SAME list — one decision per env,
// whatever the step workgroup stores meanwhile — and wave w writes part w of every listed slot (rc+vc+bookkeeping | qc+wc | qt | wt,
// as the persistent kernels' refill does: ~150-350 instructions where the whole reset has ~900), wave 0 the tags behind its part.
// Nobody reads a record in the launch that writes it (see the kernel), so parts and tag need no order among themselves.
template <typename ST>
__device__ __forceinline__ void refill_stale_slots(const StepArgs& A, const DevParams& P, int64_t base, int wv, int lane, uint32_t* job_kind,
                                                   uint32_t* job_counter, uint16_t* lists) {
  constexpr int Q = kSplitEnvs / kWave;
  constexpr int kWords = sizeof(typename Vec4<ST>::type) / 4, kWordK = kWords / 4, kWordEpisode = 3 * kWords / 4;   // .y and .w of chunk 5
  if (wv < Q) {
    const uint32_t* c5 = reinterpret_cast<const uint32_t*>(reinterpret_cast<const typename Vec4<ST>::type*>(A.ws) + 5 * A.cs);
    const int s = wv * kWave + lane;
    const int64_t ii = base + s;
    const bool ok = ii < A.n;
    const int64_t il = ok ? ii : A.n - 1;
    const uint32_t k = c5[il * kWords + kWordK], episode = c5[il * kWords + kWordEpisode], tag = A.prep_tag[il];
    job_kind[s] = (ok && k == 0u && tag != episode + 1u) ? JOB_REFILL : JOB_NONE;
    job_counter[s] = episode;
  }
  __syncthreads();
  if (wv >= Q) return;
  uint16_t* list = lists + wv * kSplitEnvs;
  bool flag[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) flag[q] = job_kind[q * kWave + lane] != JOB_NONE;
  const int total = compact_flags<Q>(flag, lane, list);
  const SlotStore<ST> S = hbm_slot_store<ST>(A.prep);
#pragma clang loop unroll(disable)
  for (int j0 = 0; j0 < total; j0 += kWave) {
    const int j = j0 + lane;
    if (j < total) {
      const int s = (int)list[j];
      const uint32_t counter = job_counter[s];
      const int64_t ii = base + s;
      slot_refill_role<ST>(wv, P, S, ii, A.seed, A.env_id_offset + (uint64_t)ii, counter, tape_row_of(A.tape, A.tape_depth, A.n, ii, counter));
      if (wv == 0) A.prep_tag[ii] = counter + 1u;
    }
  }
}

// Round 3 measured three ways of shortening what stands in front of the barrier (all bit-identical, all SLOWER; code in commits
// 794a540, 8ad2438 and 93382df, evidence under profiles/):
//  - the speculative reset split over TWO service waves per step wave (12-wave workgroup, chaser half | target half in LDS): the
//    halves' chains are shorter (5,356 and 6,436 cycles to the barrier against 6,596) and the launch takes 7.01 us against 6.78
//    (profiles/r03_split_service_waves_stamps.txt).  What bounds the time to the barrier is not either wave's chain but the SIMD's
//    vector issue: SQ_ACTIVE_INST_VALU has the step wave's ~940 and the service wave's ~900 instructions keep the VALU busy for nearly
//    all of those cycles (profiles/r03_sq_counters_closed_loop.csv);
//  - so the work itself would have to go: the step waves post, a quarter into the transition, which episodes CERTAINLY end (time limit,
//    bubble) and the service waves reset only those, by part, beside the rest of the transition (step_kernel_hint): 7.99 us.  14 % of
//    this workload's ends are attitude-error ends, known only after the chaser's attitude step — 83 % of the workgroups have one per
//    step and pay a third barrier — and a dozen-lane by-part pass takes ~4,400 cycles beside the rest of the transition, not the
//    ~1,200 its ~300 instructions suggest: its Philox blocks are quarter-rate integer multiplies on the same VALU the step wave is
//    saturating (profiles/r03_split_hint_stamps.txt);
//  - no reset arithmetic on the chain at all (step_kernel_slots, commit 93382df): prepared slots in HBM, requested by the ending lanes
//    ~40 % into the transition (branch-free), copied at the end, refilled by part beside the NEXT launch's step; no barrier: 7.49 us.
//    The step waves' transition is no faster beside nearly idle service waves (it is a dependency chain through the chaser side, not
//    an issue count: removing the whole target side from it gains 0.17 us), and the slot copy is work they did not have before
//    (profiles/r03_split_slots_hint.txt).
//
// The slot form (kSlots; fp32 storage, kAll, on_done == RESET only) is the fourth attempt at taking the speculative reset off the path to
// the barrier, and keeps everything that made this kernel win: the single barrier right behind the transition, the step waves as they
// are, the reset writes beside the step waves' statistics and outputs.  It changes the two things the slot attempts lost by:
//  - the SERVICE waves fetch the prepared slots, not the step waves: at entry every service lane requests its env's chunk 5 (k, episode)
//    and its tag, waits for them, and then — if tag == episode + 1 and k >= 1, i.e. if the slot can be consumed in this launch —
//    its env's 192-byte record (rdv_slots.h: hbm_slot_store): dense, coalesced, ~4,000 cycles before the data is used; it goes to the
//    barrier without any arithmetic.  Behind it a lane whose env finished copies the record (state chunks to HBM, observation to its
//    LDS row) if it requested one; otherwise (an env that ends on the first step of its episode, or a slot that is stale for whatever
//    reason) it runs today's in-lane reset: slow, rare, correct.  The records go out in a SECOND stage because they are the least
//    urgent requests of the CU and were the most numerous: issued at entry with everything else (54 KB per CU beside the step waves'
//    35 KB) they stood in the queues in front of the state the step waves begin with (profiles/split_prefetch_order.txt: 6.09 ->
//    5.92 us per launch at 65,536 envs; a fixed s_sleep in front of the requests gains less at every length);
//  - the refill leaves the workgroup: the grid has one more workgroup per step workgroup (blockIdx.x >= the number of step workgroups;
//    for the flagship's 256 both indices are equal mod 8: same XCD, same L2), whose waves 0-3 list — ballots, no atomics — the envs of
//    step workgroup j with k == 0 and tag != episode + 1 (~13 of 256 with random actions, all 256 after a synchronous episode end)
//    and write their slots BY PART, one part per wave (refill_stale_slots, above).  No LDS hand-off to the step workgroup, no barrier
//    shared with it, no statistics; priority 0, in the issue gaps of a step wave as the speculative reset is.  (A grid has one block
//    size: waves 4-7 of a refill workgroup end at its barrier.)  The first version ran the WHOLE reset for the listed envs on one
//    wave, in-lane: that wave began behind the dispatch of all step workgroups, waited for its loads and then had the ~900
//    instructions of a reset in front of it — it outlived the step waves and the launch took 7.27 us against 6.46; by part the refill
//    waves leave 3,970 ns after the launch's first wave (median) where the step waves leave at 4,110, and the launch takes 6.07 us.
// Why no torn record can be consumed: a record is WRITTEN only in a launch where its env has k == 0 on entry, and CONSUMED only in a
// launch where it has k >= 1 on entry — never both in one launch, and launches on a stream are ordered.  The one exception is a refill
// wave that runs late and already sees the new episode (k == 0) of an env that finished in this very launch: that write comes after
// the consumer has loaded the record and stored the state, and the next launch rewrites it identically or finds the tag current.  A
// slot that is stale while k >= 1 is deliberately NOT refilled in-kernel: its env falls back when it ends and is refilled one launch
// later.  Launches that advance episodes without maintaining the slots (every other rdv_step kernel) and calls that change what a
// reset returns clear the handle's step_slots_ok; prepare_kernel then runs in front of the next slot-form launch (rdv_hip.hip).
// Measured: profiles/split_slots_prefetch.txt.
//
// The target form (kTarget; the slot form's conditions, its refill workgroups and its reset paths unchanged) gives the service wave, which
// in the slot form only waits in front of the barrier, the part of the transition that depends on nothing the step wave computes: the
// target's attitude step (step_target), the rounding of qt, R(qt) and R(qt) rd (derive_target_head) — the same functions on the same
// inputs, so the same bits.  The service wave loads chunks 4 and 6 with its first stage (the step wave no longer requests them: the
// bytes requested at entry per CU are the same), posts qt as four floats, R(qt) rd as three doubles and wt as three floats in LDS
// ([component][env], 52 bytes per env), and requests the slot records BEHIND the join, so that nothing but the second barrier stands
// between the untracked record loads and their wait (no instruction there that could move a record register; the requests in front of
// the arithmetic, with a dozen live record registers across it, were not built).  The step wave runs step_env_chaser, JOINS at a
// workgroup barrier, and finishes from the posted values (step_env_finish<.., kHanded>: the lazy branches rebuild R(qt), the reward —
// the one consumer of the table entry requested at the end of the chaser half — comes last; the entry is requested with a GLOBAL load
// there, because a flat load counts as an LDS operation and the join's wait for LDS would wait for it).  Every wave of a step workgroup
// executes exactly two barriers, on every path: the join, and the barrier behind the termination ballot; the refill workgroups are the
// slot form's.  Measured (profiles/split_target_on_service.txt, tools/lib_ab.py, us per launch, slot form -> this form): 5.93 -> 5.71 at
// 65,536 envs, 5.59 -> 5.27 at 32,768, 5.10 -> 4.79 at 16,384; the stamped build has the service wave post 2,160 cycles after entry and
// wait 1,430 at the join, the step wave arrive at 3,520 and wait 56.  The default form wherever the slot form runs (split_target_by_size).
// The two older forms now run through the same body function, which changed their instruction streams by operand order and a few
// instructions (profiles/split_target_isa_diff.md): the slot form measures 5.97 us that way, 0.04 more than before.
#ifndef RDV_TARGET_SERVICE_PRIO
// s_setprio of the service wave's arithmetic segment; the step waves run at 2.  Above them it wins: the first stage lands while the step wave
// still waits for its state, and what fits there is free — 5.74 us per launch at 0 and at 1, 5.71 at 3 (65,536 envs, four children each)
#define RDV_TARGET_SERVICE_PRIO 3
#endif
// The twelve requests of a slot record (fp32 storage: 12 vectors) as ONE statement under an exec mask it saves and restores itself; see the
// service waves of the slot form.  A macro, not a function or a lambda: the statement stands at one of two places by form, and as a
// lambda the older forms' register allocation changed (their instruction streams are held to the parent's: profiles/split_obs_isa_diff.md).
#define RDV_REQUEST_RECORDS(rec, recp, mask, saved)                                                                                                  \
  do {                                                                                                                                               \
    _Pragma("unroll") for (int v_ = 0; v_ < 12; ++v_) asm volatile("" : "=v"(rec[v_]));   /* defined registers for the lanes that request nothing */   \
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t"                                                                                                \
                 "global_load_dwordx4 %[r0], %[p], off\n\t"                                                                                          \
                 "global_load_dwordx4 %[r1], %[p], off offset:16\n\t"                                                                                \
                 "global_load_dwordx4 %[r2], %[p], off offset:32\n\t"                                                                                \
                 "global_load_dwordx4 %[r3], %[p], off offset:48\n\t"                                                                                \
                 "global_load_dwordx4 %[r4], %[p], off offset:64\n\t"                                                                                \
                 "global_load_dwordx4 %[r5], %[p], off offset:80\n\t"                                                                                \
                 "global_load_dwordx4 %[r6], %[p], off offset:96\n\t"                                                                                \
                 "global_load_dwordx4 %[r7], %[p], off offset:112\n\t"                                                                               \
                 "global_load_dwordx4 %[r8], %[p], off offset:128\n\t"                                                                               \
                 "global_load_dwordx4 %[r9], %[p], off offset:144\n\t"                                                                               \
                 "global_load_dwordx4 %[r10], %[p], off offset:160\n\t"                                                                              \
                 "global_load_dwordx4 %[r11], %[p], off offset:176\n\t"                                                                              \
                 "s_mov_b64 exec, %[sv]"                                                                                                             \
                 : [r0] "+v"(rec[0]), [r1] "+v"(rec[1]), [r2] "+v"(rec[2]), [r3] "+v"(rec[3]), [r4] "+v"(rec[4]), [r5] "+v"(rec[5]), [r6] "+v"(rec[6]), \
                   [r7] "+v"(rec[7]), [r8] "+v"(rec[8]), [r9] "+v"(rec[9]), [r10] "+v"(rec[10]), [r11] "+v"(rec[11]), [sv] "=&s"(saved)               \
                 : [p] "v"(recp), [m] "s"(mask)                                                                                                      \
                 : "scc");                                                                                                                           \
  } while (0)
// The body of both kernels below.  kAll: on_done != HALT — every lane of the step waves runs the transition (advance_all).
// stage / fin_mask: the kernel's LDS (observation rows [256][17]; per step wave, the lanes to reset).  hand_f / hand_d: the target form's
// hand-over in LDS ([7][256] floats: qt, wt; [3][256] doubles: R(qt) rd), null otherwise.  hand_c / out_mask: the observation form's
// hand-over the other way ([13][256] floats: the canonical rc, vc, qc, wc of the chaser half) and, per step wave, the service wave's ballot
// of the lanes whose observation lies outside the Box; null otherwise.
template <typename ST, bool kAll, bool kSlots, bool kTarget, bool kObs = false>
__device__ __forceinline__ void split_body(void* ws_hot, const float* actions_hot, const DevParams* Pp, int64_t n_hot, uint64_t* stats_hot, float* obs_hot,
                                           float* reward_hot, const StepArgs& A_rest, float* stage, unsigned long long* fin_mask, float* hand_f, double* hand_d,
                                           float* hand_c = nullptr, unsigned long long* out_mask = nullptr) {
  static_assert(!kTarget || kSlots, "the target form is a form of the slot form");
  static_assert(!kObs || kTarget, "the observation form is a form of the target form");
  constexpr int kS = kTarget ? 1 : 0;   // stamps (diagnostic build): the target form has 2 = at the join, 3 = past it, and the later ones one up
  (void)kS; (void)hand_f; (void)hand_d; (void)hand_c; (void)out_mask;
  const StepArgs A = hot_args(A_rest, ws_hot, actions_hot, n_hot, stats_hot, obs_hot, reward_hot);
  using V = typename Vec4<ST>::type;
  const DevParams& P = *Pp;   // scalar loads: see step_kernel
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = threadIdx.x >> 6;
  const bool step_role = wv < kSplitEnvs / kWave;
  const int slot_in_block = threadIdx.x & (kSplitEnvs - 1);          // both roles: the env this lane is responsible for
  const int64_t n = A.n;
  const int64_t i = (int64_t)blockIdx.x * kSplitEnvs + slot_in_block;
  const int64_t wave_base = i - lane;
  const bool active = i < n;
  const int64_t rows = (n - wave_base) < kWave ? (n - wave_base) : kWave;
  V* ws = reinterpret_cast<V*>(A.ws);
  const bool resets = A.on_done == RDV_ON_DONE_RESET;
  RDV_STAMP_DECL
  RDV_STAMP(0);

  if constexpr (kSlots) {
    static_assert(sizeof(ST) == 4 && kAll, "the slot form is built for fp32 storage without halted envs");
    // ------------------------------------------------------------------ refill workgroups
    const unsigned n_step_wgs = (unsigned)((n + kSplitEnvs - 1) / kSplitEnvs);
    const bool refill_role = blockIdx.x >= n_step_wgs;
    const unsigned refill_wg = blockIdx.x - n_step_wgs;
    if (refill_role) {
      uint32_t* words = reinterpret_cast<uint32_t*>(stage);
      refill_stale_slots<ST>(A, P, (int64_t)refill_wg * kSplitEnvs, wv, lane, words, words + kSplitEnvs, reinterpret_cast<uint16_t*>(words + 2 * kSplitEnvs));
      if (wv == 0) {
        RDV_STAMP(7);
        RDV_STAMP_FLUSH(((uint64_t)refill_wg + n_step_wgs) * 8)
      }
      return;
    }
  }
  if (step_role) {
    // ------------------------------------------------------------------ step waves
    __builtin_amdgcn_s_setprio(2);   // (the longer of the SIMD's two instruction streams first: 6.43 -> 6.41 us per launch; the service waves first: 7.03)
    float* wl = stage + wv * (kWave * RDV_OBS_DIM);
    Env e;
    StepResult r;
    uint64_t* slot = A.stats + (uint64_t)(wave_base / kWave) * kStatWords;
    uint64_t slot_pre;
    float a[RDV_ACT_DIM];
    constexpr bool kPinned = kAll && sizeof(ST) == 4;
    PinnedInputs pin;
    if constexpr (kPinned) {
      // state chunks, action row and statistics slot requested together (rdv_kernels.h: PinnedInputs); the state is waited for here, the
      // action row behind the chaser's rotation matrix (actions_ready).  kTarget: without chunks 4 and 6, which the service wave loads
      pinned_state<kTarget>(A, wave_base, lane, pin, e);
    } else if constexpr (kAll) {
      TileInputs<ST> in;
      tile_fetch<ST>(A, wave_base, lane, in);
      unpack_env<ST>(in.c, e);
      slot_pre = in.slot_pre;
#pragma unroll
      for (int k = 0; k < 3; ++k) { a[2 * k] = in.a[k].x; a[2 * k + 1] = in.a[k].y; }
    } else {
      if (active) load_env<ST>(ws, A.cs, i, e);
      slot_pre = stats_preload(slot, lane);
      load_actions(A.actions, wave_base, lane, active, a);
    }
    RDV_STAMP_STATE(e);
    RDV_STAMP(1);
    // observation rows: own row -> LDS as it is formed (stride 17: conflict-free) -> contiguous stores.  If an env of this wave
    // resets, the rows stay in LDS: the service wave swaps in the reset observation and stores the block — which is why this kernel
    // also keeps the row in registers: after the barrier the LDS row may already hold the next episode's observation when the terminal
    // one is stored (one wave per SIMD here: the 17 registers cost no occupancy).
    float obs_r[RDV_OBS_DIM];
    float* my_row = wl + lane * RDV_OBS_DIM;
    constexpr bool kPack = sizeof(ST) == 4;   // fp32 storage: pack inside the stepped branch (advance()); fp64 storage has nothing to convert — there the
    V packed[kChunks];                        // 56 extra registers of a packed copy cost 0.4 us per launch (8.75 -> 9.17 measured), so it stores from `e`
    auto row_sink = [&](int j, float v) { obs_r[j] = v; my_row[j] = v; };
    bool stepped;
    auto actions_ready = [&](double& after) { if constexpr (kPinned) pinned_rest(pin, after, a, slot_pre); };
    if constexpr (kTarget) {
      // advance_all in its halves: the chaser half, the join, the finish from what the service wave posted
      r.done = 0; r.reason = 0; r.reward = 0.0f; r.reward64 = 0.0;
      Derived d;
      StepCtx c;
      step_env_chaser<ST, false, false, true>(P, e, a, d, c, actions_ready);   // (the table entry by a global load: the join must not wait for it)
      if constexpr (kObs) {
        // the chaser half is final here: canonical values, floats under fp32 storage, so the service wave's (double)(float) is exact
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          hand_c[k * kSplitEnvs + slot_in_block] = (float)e.rc[k];
          hand_c[(3 + k) * kSplitEnvs + slot_in_block] = (float)e.vc[k];
          hand_c[(10 + k) * kSplitEnvs + slot_in_block] = (float)e.wc[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) hand_c[(6 + k) * kSplitEnvs + slot_in_block] = (float)e.qc[k];
      }
      RDV_STAMP(2);
      __syncthreads();   // the join: the service waves have posted the target side of this workgroup's envs
      RDV_STAMP(3);
      double rd_l[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) e.qt[k] = (double)hand_f[k * kSplitEnvs + slot_in_block];   // canonical: (double)(float) as canon() forms it
#pragma unroll
      for (int k = 0; k < 3; ++k) { e.wt[k] = (double)hand_f[(4 + k) * kSplitEnvs + slot_in_block]; rd_l[k] = hand_d[k * kSplitEnvs + slot_in_block]; }
      if constexpr (kObs) step_env_finish<ST, true, false, true, true>(P, e, r, d, c, NoHook(), rd_l);   // r.done, r.reason: time | bubble | attitude
      else step_env_finish<ST, true, false, true>(P, e, r, d, c, row_sink, rd_l);
      pack_env<ST>(e, packed);
      stepped = active;
    } else {
      if constexpr (kAll) { advance_all<ST>(P, e, a, r, row_sink, kPack ? packed : nullptr, actions_ready); stepped = active; }
      else stepped = advance<ST, false>(A, P, i, active, e, a, r, row_sink, NoHook(), kPack ? packed : nullptr);
      RDV_STAMP(2);
    }
    bool fin = stepped && r.done;          // (kObs: by the three tests of this wave; the Box test's share arrives behind the barrier)
    bool to_reset = fin && resets;
    const unsigned long long m_reset = __ballot(to_reset);
    if (lane == 0) fin_mask[wv] = m_reset;
    // The barrier comes HERE, as soon as the service waves have what they wait for (which envs ended, the observation rows), not at the
    // end of the step wave: the statistics, the per-env outputs and the stores of the step wave (~1.1 us) then run beside the service
    // waves' reset writes (~0.9 us) instead of in front of them (stamps: 5.7 -> ~5.0 us from the first wave's entry to the last exit).
    // The state of the envs that go on is stored BEFORE the barrier (round 3): the step waves reach it ~700 cycles ahead of the service
    // waves, and these 6 x 16-byte-per-lane stores drain inside that wait instead of after it (tools/lib_ab.py: 6.80 -> 6.73 us at
    // 65,536 envs, 5.35 -> 5.29 at 16,384; moving the reward / done / terminal-row stores there as well loses: 6.89).  Reset lanes: service wave.
    if constexpr (!kObs) {
      halt_if_done<ST>(A, fin, e, kPack ? packed : nullptr);
      if (stepped && !to_reset) { if (kPack) store_chunks<ST, true>(ws, A.cs, i, packed, false); else store_env<ST>(ws, A.cs, i, e, false); }
    }
    RDV_STAMP(3 + kS);
    __syncthreads();
    RDV_STAMP(4 + kS);
    if constexpr (kObs) {
      // The termination decision is assembled from two waves: this one has posted the ballot of its three tests, the service wave the
      // ballot of the Box test of the observation it formed (masked by `active`, as `stepped` is here).  Who goes on is known only now, so
      // the state stores of those envs come behind the barrier, first of all.  (A third barrier in front of this decision, which keeps them
      // in front of the last one as in the target form, measures 0.06 us slower: profiles/split_obs_on_service.txt.)
      if ((out_mask[wv] >> lane) & 1ull) { r.done = 1; r.reason = 1; }       // :381 first true: outside comes first
      fin = stepped && r.done;
      to_reset = fin && resets;
      halt_if_done<ST>(A, fin, e, packed);
      if (stepped && !to_reset) store_chunks<ST, true>(ws, A.cs, i, packed, false);
    }
    stats_update(slot, slot_pre, lane, stepped, fin, r.reason, e.flags, e.k, e.ep_ret, e.sum_dv, e.sum_dw);
    if constexpr (kObs) {
      store_step_outputs<false>(A, i, active, fin, r, e, nullptr);            // terminal rows and observation rows: the service wave
    } else {
      store_step_outputs<true>(A, i, active, fin, r, e, obs_r);
      if (m_reset == 0ull) store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);
    }
    RDV_STAMP(5 + kS);
    RDV_STAMP(6 + kS);
  } else if constexpr (kSlots) {
    // ------------------------------------------------------------------ service waves, slot form
    // The requests in the order of their urgency (profiles/split_prefetch_order.txt).  Every lane first requests its env's chunk 5 (k,
    // episode) and its tag (the index is clamped into the batch, as in tile_fetch) and waits for them: one round trip to L2, in which
    // the step waves' ten input requests of this CU — and of the workgroups dispatched a little earlier on the XCD — are served
    // without 12 x 16 bytes per service lane queued in front of them.  The wait is the delay: no constant to tune.  Then the lanes whose
    // slot CAN be consumed in this launch (tag == episode + 1 and k >= 1: `copy_ok`, the one value that also picks the copy path behind
    // the barrier, so a lane that requested nothing cannot copy) request the twelve vectors of the record, all in flight together,
    // ~4,000 cycles before the barrier.  The other lanes (k == 0: ~5 % with random actions, and their records are the ones the refill
    // workgroup is writing in this launch) request nothing.  Loads and waits are inline assembly with the registers as operands, as
    // PinnedInputs' are (rdv_kernels.h): written as C++ loads the compiler hoists the record requests back in front of the wait.  The
    // record requests are ONE statement under an exec mask it saves and restores itself: no branch, and no place for the compiler to put
    // a copy of a register whose data has not landed.
    constexpr int kRecVecs = kChunks + kSlotObsVecs;
    static_assert(slot_record_bytes<ST>() == kRecVecs * 16 && kRecVecs == 12, "the fp32 slot record is 12 vectors: the requests are written out below");
    const int64_t il = active ? i : n - 1;
    const pin_f4* recp = reinterpret_cast<const pin_f4*>(A.prep) + il * kRecVecs;
    pin_f4 rec[kRecVecs];
    pin_f4 c5;
    uint32_t tag;
    // observation form: the env this lane forms the observation of (rc, vc, qc, wc from the step wave's post, qt its own), the row in
    // registers for the terminal rows (the staged row is overwritten by the reset observation), the Box test
    Env obs_env;
    float obs_r[RDV_OBS_DIM];
    bool obs_outside = false;
    (void)obs_env; (void)obs_r; (void)obs_outside;
    if constexpr (kTarget) {
      // the first stage also brings the target's chunks 4 (qt) and 6 (wt), which the step wave no longer requests; behind the wait the
      // target side of the transition runs here, beside the step wave's chaser half, and is posted for the join
      pin_f4 c4, c6;
      const pin_f4* wsl = reinterpret_cast<const pin_f4*>(ws) + il;
      asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %5, off\n\tglobal_load_dwordx4 %2, %6, off\n\tglobal_load_dword %3, %7, off"
                   : "=&v"(c4), "=&v"(c6), "=&v"(c5), "=&v"(tag) : "v"(wsl + 4 * A.cs), "v"(wsl + 6 * A.cs), "v"(wsl + 5 * A.cs), "v"(A.prep_tag + il));
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(c4), "+v"(c6), "+v"(c5), "+v"(tag));
      RDV_STAMP(1);
      if (RDV_TARGET_SERVICE_PRIO) __builtin_amdgcn_s_setprio(RDV_TARGET_SERVICE_PRIO);
      double qt[4] = {c4.x, c4.y, c4.z, c4.w}, wt[3] = {c6.x, c6.y, c6.z};
      step_target<false, false>(P, qt, wt);       // :184 (wt is constant under the reference's bodies: handed over as loaded)
      double Rt[9], rd_l[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) qt[k] = canon(qt[k], ST(0));
      derive_target_head(P, qt, Rt, rd_l);
#pragma unroll
      for (int k = 0; k < 4; ++k) hand_f[k * kSplitEnvs + slot_in_block] = (float)qt[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) { hand_f[(4 + k) * kSplitEnvs + slot_in_block] = c6[k]; hand_d[k * kSplitEnvs + slot_in_block] = rd_l[k]; }
      if constexpr (kObs) {
        // the observation's last four elements are this wave's own canonical qt: formed here, in the wait for the join
#pragma unroll
        for (int k = 0; k < 4; ++k) obs_env.qt[k] = qt[k];
        float* my_row = stage + slot_in_block * RDV_OBS_DIM;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = (float)obs_env.qt[k];
          obs_outside |= !(fabsf(v) <= 1.0f);
          obs_r[13 + k] = v; my_row[13 + k] = v;
        }
      }
      if (RDV_TARGET_SERVICE_PRIO) __builtin_amdgcn_s_setprio(0);
    } else {
      asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dword %1, %3, off"
                   : "=&v"(c5), "=&v"(tag) : "v"(reinterpret_cast<const pin_f4*>(ws) + 5 * A.cs + il), "v"(A.prep_tag + il));
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(c5), "+v"(tag));
      RDV_STAMP(1);
    }
    const uint32_t k_in = __float_as_uint(c5.y), episode_in = __float_as_uint(c5.w);
    const bool copy_ok = tag == episode_in + 1u && k_in >= 1u;
    // The twelve record requests.  Slot and target form: behind the inputs / behind the join, with nothing but the barrier between them and their
    // wait.  Observation form: in FRONT of the join, in the wait for the step wave (1,400 cycles in which this wave issues nothing), so
    // that the observation arithmetic behind the join starts at once; the 48 record registers are then in flight, untracked, across the
    // join and that arithmetic — the compiler sees them as live values and has no reason to touch them, and that it does not is read in
    // the ISA (profiles/split_obs_on_service.txt: behind the join 5.79 us per launch at 65,536 envs, in front of it 5.72).
    unsigned long long saved_exec;
    if constexpr (kObs) RDV_REQUEST_RECORDS(rec, recp, __ballot(copy_ok), saved_exec);
    if constexpr (kTarget) {
      // The join.  The target form's record requests go out BEHIND it: nothing but the second barrier then stands between the untracked
      // loads and their wait, as in the slot form, and they have the step waves' whole finish to land in.
      RDV_STAMP(2);
      __syncthreads();
      RDV_STAMP(3);
    }
    if constexpr (!kObs) RDV_REQUEST_RECORDS(rec, recp, __ballot(copy_ok), saved_exec);
    if constexpr (kObs) {
      // The observation, beside the step wave's finish: observation_to on the posted chaser values (elements 0..12; 13..16 are in the row
      // already), every element into the env's staged row and into a register, the Box test as step_env_finish makes it, and the wave's
      // ballot of it for the step wave.
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        obs_env.rc[k] = (double)hand_c[k * kSplitEnvs + slot_in_block];
        obs_env.vc[k] = (double)hand_c[(3 + k) * kSplitEnvs + slot_in_block];
        obs_env.wc[k] = (double)hand_c[(10 + k) * kSplitEnvs + slot_in_block];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) obs_env.qc[k] = (double)hand_c[(6 + k) * kSplitEnvs + slot_in_block];
      float* my_row = stage + slot_in_block * RDV_OBS_DIM;
      observation_to(P, obs_env, [&](int j, float v) {
        if (j >= 13) return;
        obs_outside |= !(fabsf(v) <= 1.0f);                                                // Box.contains; NaN -> outside
        obs_r[j] = v; my_row[j] = v;
      });
      const unsigned long long m_out = __ballot(active && obs_outside);
      if (lane == 0) out_mask[wv - kSplitEnvs / kWave] = m_out;
    }
#ifdef RDV_STAMPS
    if constexpr (!kObs)   // (the observation form's stamp at the barrier is "the Box test is posted": its records stay in flight, as in the product)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2]), "+v"(rec[3]), "+v"(rec[4]), "+v"(rec[5]), "+v"(rec[6]),
                 "+v"(rec[7]), "+v"(rec[8]), "+v"(rec[9]), "+v"(rec[10]), "+v"(rec[11]));   // stamps build only: stamp 2 is "the records have landed"
#endif
    if constexpr (!kTarget) RDV_STAMP(2);
    RDV_STAMP(3 + kS);
    __syncthreads();
    RDV_STAMP(4 + kS);
    // the compiler does not track these loads: every use of a record register it sees is of the value behind this wait
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec[0]), "+v"(rec[1]), "+v"(rec[2]), "+v"(rec[3]), "+v"(rec[4]), "+v"(rec[5]), "+v"(rec[6]),
                 "+v"(rec[7]), "+v"(rec[8]), "+v"(rec[9]), "+v"(rec[10]), "+v"(rec[11]));
    unsigned long long m_reset = fin_mask[wv - kSplitEnvs / kWave];
    if constexpr (kObs) m_reset |= out_mask[wv - kSplitEnvs / kWave];   // time | bubble | attitude by the step wave, the Box test by this one
    if (m_reset != 0ull) {   // wave-uniform: some env of the step wave we serve finished its episode
      float* wl = stage + (wv - kSplitEnvs / kWave) * (kWave * RDV_OBS_DIM);
      if (active && ((m_reset >> lane) & 1ull)) {
        if constexpr (kObs) {
          // the terminal row, from the registers: the staged row is about to take the next episode's first observation
          if (A.terminal_obs) {
            float* t = A.terminal_obs + i * RDV_OBS_DIM;
#pragma unroll
            for (int j = 0; j < RDV_OBS_DIM; ++j) t[j] = obs_r[j];
          }
        }
        if (copy_ok) {
          // copy path: the record is reset(seed, id, episode_in), state chunks in storage layout + observation
          if (__float_as_uint(rec[5].z) == kFlagsPending) {   // refilled by part (persistent kernels): the flags need the whole state
            float4 c[kChunks];
#pragma unroll
            for (int j = 0; j < kChunks; ++j) c[j] = make_float4(rec[j].x, rec[j].y, rec[j].z, rec[j].w);
            Env se;
            unpack_env<float>(c, se);
            rec[5].z = __uint_as_float(reset_flags(P, se));
          }
          pin_f4* dst = reinterpret_cast<pin_f4*>(ws) + i;
#pragma unroll
          for (int j = 0; j < kChunks; ++j) __builtin_nontemporal_store(rec[j], dst + j * A.cs);
#pragma unroll
          for (int j = 0; j < RDV_OBS_DIM; ++j) wl[lane * RDV_OBS_DIM + j] = rec[kChunks + (j >> 2)][j & 3];
        } else {
          // fallback path: today's reset, in-lane
          Env ne;
          float robs[RDV_OBS_DIM];
          ne.episode = episode_in;
          const double* row = nullptr;
          if (A.tape_depth > 0) row = A.tape + ((int64_t)(ne.episode % (uint32_t)A.tape_depth) * n + i) * RDV_STATE_DIM;
          reset_state<ST, false>(P, ne, A.seed, A.env_id_offset + (uint64_t)i, row);
          reset_aux<ST>(P, ne);
          canon_rest<ST>(ne);
          observation(P, ne, robs);
          store_env<ST, true>(ws, A.cs, i, ne, true);
#pragma unroll
          for (int j = 0; j < RDV_OBS_DIM; ++j) wl[lane * RDV_OBS_DIM + j] = robs[j];
        }
      }
      if constexpr (!kObs) {
        wave_lds_fence();
        RDV_STAMP(5 + kS);
        store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);
      }
    }
    if constexpr (kObs) {   // the rows are this wave's in every case: it staged them
      wave_lds_fence();
      RDV_STAMP(5 + kS);
      store_obs_rows<true>(A.obs, wave_base, rows, lane, stage + (wv - kSplitEnvs / kWave) * (kWave * RDV_OBS_DIM));
    }
    RDV_STAMP(6 + kS);
  } else {
    // ------------------------------------------------------------------ service waves
    // The observation and the storage packing of the next initial state are computed after the barrier, by the lanes that use them:
    // since the action rows stopped travelling through LDS the service waves are the last to reach the barrier (stamps: ~7,100
    // cycles after entry against ~5,800 for the step waves), and every instruction taken out of their path before it counts
    // (tools/lib_ab.py: 6.88 -> 6.78 us per launch at 65,536 envs, 5.58 -> 5.36 at 16,384).  Deferring more — the target's rate, with
    // its rotation matrix — overshoots: 7.05 us.
    Env ne;
    if (resets && active) {
      const V c5 = ws[5 * A.cs + i];
      ne.episode = s2u(c5.w);
      RDV_STAMP(1);
      const double* row = nullptr;   // (tape_row_of without its opaque divisor, which would change this wave's instruction stream)
      if (A.tape_depth > 0) row = A.tape + ((int64_t)(ne.episode % (uint32_t)A.tape_depth) * n + i) * RDV_STATE_DIM;
      reset_state<ST, false>(P, ne, A.seed, A.env_id_offset + (uint64_t)i, row);   // rounded to the storage type below, where a state is taken
      reset_aux<ST>(P, ne);
      RDV_STAMP(2);
    }
    RDV_STAMP(3);
    __syncthreads();
    RDV_STAMP(4);
    const unsigned long long m_reset = fin_mask[wv - kSplitEnvs / kWave];
    if (m_reset != 0ull) {   // wave-uniform: some env of the step wave we serve finished its episode
      float* wl = stage + (wv - kSplitEnvs / kWave) * (kWave * RDV_OBS_DIM);
      if (active && ((m_reset >> lane) & 1ull)) {
        float robs[RDV_OBS_DIM];
        canon_rest<ST>(ne);
        observation(P, ne, robs);
        store_env<ST, true>(ws, A.cs, i, ne, true);
#pragma unroll
        for (int j = 0; j < RDV_OBS_DIM; ++j) wl[lane * RDV_OBS_DIM + j] = robs[j];
      }
      wave_lds_fence();
      RDV_STAMP(5);
      store_obs_rows<true>(A.obs, wave_base, rows, lane, wl);
    }
    RDV_STAMP(6);
  }
  RDV_STAMP(7);
  RDV_STAMP_FLUSH((uint64_t)blockIdx.x * 8 + wv)
}

template <typename ST, bool kAll, bool kSlots = false>
__global__ __launch_bounds__(kSplitBlock) void step_kernel_split(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                       uint64_t* stats_hot, float* obs_hot, float* reward_hot, const StepArgs A_rest) {
  __shared__ __attribute__((aligned(16))) float stage[kSplitEnvs * RDV_OBS_DIM];   // observation rows
  __shared__ unsigned long long fin_mask[kSplitEnvs / kWave];                        // per step wave: lanes to reset
  split_body<ST, kAll, kSlots, false>(ws_hot, actions_hot, Pp, n_hot, stats_hot, obs_hot, reward_hot, A_rest, stage, fin_mask, nullptr, nullptr);
}

// The target form: a kernel of its own name (the launch still reports "step_kernel_split<float, true>": it is a form of that kernel, picked
// like the slot form), with the 13 KB of the hand-over beside the observation rows — 30,752 bytes of LDS per workgroup, so a step and a
// refill workgroup still share a CU.
template <typename ST>
__global__ __launch_bounds__(kSplitBlock) void step_kernel_split_target(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                              uint64_t* stats_hot, float* obs_hot, float* reward_hot, const StepArgs A_rest) {
  __shared__ __attribute__((aligned(16))) float stage[kSplitEnvs * RDV_OBS_DIM];   // observation rows
  __shared__ unsigned long long fin_mask[kSplitEnvs / kWave];                        // per step wave: lanes to reset
  __shared__ double hand_d[3 * kSplitEnvs];   // R(qt) rd, [component][env]
  __shared__ float hand_f[7 * kSplitEnvs];    // canonical qt, then wt
  split_body<ST, true, true, true>(ws_hot, actions_hot, Pp, n_hot, stats_hot, obs_hot, reward_hot, A_rest, stage, fin_mask, hand_f, hand_d);
}

// The observation form (kObs; the target form's conditions, refill workgroups, slot rules and reset paths unchanged) also gives the service
// wave the observation, the largest piece of the step wave's finish that reads nothing the finish computes: nine normalized() elements,
// eight conversions, seventeen row writes and seventeen Box tests, ~125 of its ~330 instructions.  The step wave posts its canonical rc,
// vc, qc and wc at the end of the chaser half ([13][256] floats, 13,312 B more: 44,096 B per workgroup, a step and a refill workgroup still
// share a CU); the service wave requests the records in its wait for the join and behind it runs observation_to on the posted values and
// its own qt — the same function on the same inputs, the same bits — into the staged row and into registers, and posts the ballot of the
// Box test.  The step wave runs step_env_finish without the observation and posts the ballot of its three tests; behind the barrier both
// roles form the mask of the envs that ended, the step wave puts `outside` in front of its own reason and stores the state of the envs that
// go on, the service wave stores the terminal rows from its registers, copies or resets as before, and stores the observation rows in
// every case.  Every wave of a step workgroup executes exactly two barriers on every path.
// Measured (profiles/split_obs_on_service.txt, tools/lib_ab.py, us per launch, target form -> this form, two sessions): 5.68 -> 5.61 and
// 5.70 -> 5.64 at 65,536 envs, 5.26 -> 5.06 at 32,768, 4.80 -> 4.60 at 16,384.  Stamped, the step wave's stretch from the join to the
// barrier shrinks from 2,680 to 1,280 cycles and the barrier is reached 900 cycles earlier; most of that is paid back at 65,536 envs: the
// service wave's tail grows by the terminal rows (~570 cycles), and the refill waves, which run in the same SIMDs' issue gaps, leave
// 400-900 ns later, last of the launch.  With the requests behind the join, as the target form has them, the form LOSES at 65,536 envs
// (5.77 against 5.68: the service wave is then the last at the barrier by 590 cycles); a third barrier that keeps the state stores in
// front of the last one loses 0.06 more; s_setprio 0, 1, 3 on the observation segment measure the same, none is set.  The default
// wherever the target form runs (split_obs_by_size).
template <typename ST>
__global__ __launch_bounds__(kSplitBlock) void step_kernel_split_obs(void* ws_hot, const float* actions_hot, const DevParams* __restrict__ Pp, int64_t n_hot,
                                                           uint64_t* stats_hot, float* obs_hot, float* reward_hot, const StepArgs A_rest) {
  __shared__ __attribute__((aligned(16))) float stage[kSplitEnvs * RDV_OBS_DIM];   // observation rows
  __shared__ unsigned long long fin_mask[kSplitEnvs / kWave];                        // per step wave: lanes that ended by time, bubble or attitude
  __shared__ unsigned long long out_mask[kSplitEnvs / kWave];                        // per step wave: lanes whose observation is outside the Box
  __shared__ double hand_d[3 * kSplitEnvs];   // R(qt) rd, [component][env]
  __shared__ float hand_f[7 * kSplitEnvs];    // canonical qt, then wt
  __shared__ float hand_c[13 * kSplitEnvs];   // canonical rc, vc, qc, wc: the chaser half, for the service wave
  split_body<ST, true, true, true, true>(ws_hot, actions_hot, Pp, n_hot, stats_hot, obs_hot, reward_hot, A_rest, stage, fin_mask, hand_f, hand_d, hand_c, out_mask);
}

}  // namespace rdv

#!/usr/bin/env python3
"""Diagnostic (not product): where a launch of the split step kernel spends its time.

Builds a -DRDV_STAMPS copy of the library into tools/_stamps.so, runs a few hundred steps at N envs and prints, per role
(step waves / service waves), the median shader-cycle counts between the stamps
  0 entry | 1 inputs staged | 2 step / next-state computed | 3 at the barrier | 4 past it | 5 | 6 | 7 end
(service waves of the slot form: 1 chunk 5 and tag landed, record requests go out | 2 the records have landed — this build waits for them there)
plus, from s_memrealtime (100 MHz, one counter for the whole chip): the shader clock, when waves enter and leave
relative to the first wave of the launch, and the span of the launch as the waves see it.
RDV_SPLIT_FORM=speculative|slots|slots_target|slots_target_obs picks the form (csrc/rdv_step.h); in the slot forms the second half of the grid is the refill workgroups;
the lifetime of their wave 0 (it writes the largest part and the tags) is printed beside the two roles.  RDV_STAMPS_PREBUILT=1 uses tools/_stamps.so
(or the library RDV_STAMPS_LIB names) as it stands.
The target form (slots_target) has a join in front of the barrier, and its stamps are
  0 entry | 1 inputs staged (service waves: first stage landed, chunks 4 and 6 with it) | 2 at the join (step waves: chaser half done; service
  waves: target side posted) | 3 past the join | 4 at the barrier (service waves of this build: the records, requested behind the join, have
  landed) | 5 past it | 6 | 7 end
so phase 2>3 is what a role waits at the join; the join's line is printed beside the barrier's.
The observation form (slots_target_obs) has the target form's stamps; its service waves form the observation in phase 3>4 (this build
does not wait for the records there: they are in flight across that arithmetic, as in the product), so "at the barrier" is when the
service wave's `outside` post has landed, and its step waves store the state of the envs that go on in phase 5>6, behind the barrier.
Never quote this build's run time: the stamps fence the scheduler."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    svc = 1          # service waves per step wave (round 3 also stamped a 12-wave workgroup with two: profiles/r03_split_service_waves_stamps.txt)
    wpg = 4 * (1 + svc)
    lib = os.environ.get("RDV_STAMPS_LIB") or os.path.join(ROOT, "tools", "_stamps.so")
    target_form = os.environ.get("RDV_SPLIT_FORM", "slots_target") in ("slots_target", "slots_target_obs")      # the library's default form (a library from before it: RDV_SPLIT_FORM=slots)
    k_barrier = 4 if target_form else 3          # the stamp "at the barrier"
    from _build import build_variant
    if not os.environ.get("RDV_STAMPS_PREBUILT"):
        build_variant(lib, ["-DRDV_STAMPS"] + os.environ.get("RDV_EXTRA_FLAGS", "").split())
    import torch
    from reinforcement_learning_rendezvous_amd import _native
    _native.LIB_PATH = lib
    from reinforcement_learning_rendezvous_amd.batch import RendezvousBatch
    env = RendezvousBatch(n, device="cuda:0", storage="f32", seed=0, variant="split")
    L = _native.lib()
    L.rdv_debug_set_stamps.argtypes = [C.c_void_p, C.c_void_p]
    waves = (n + 255) // 256 * wpg
    stamps = torch.zeros((2 * waves, 10), dtype=torch.int64, device="cuda:0")      # (the slot form's refill workgroups: the second half)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    acts = [(torch.rand((n, 6), device="cuda:0", generator=gen) * 2 - 1).contiguous() for _ in range(8)]
    env.reset()
    for t in range(100):
        env.step(acts[t % 8])
    _native.check(L.rdv_debug_set_stamps(env._h, stamps.data_ptr()))
    rows = []
    for t in range(50):
        for _ in range(4):                 # back-to-back launches; the last one's stamps are read
            env.step(acts[t % 8])
        torch.cuda.synchronize()
        rows.append(stamps.cpu().numpy().copy())
    s_all = np.stack(rows).astype(np.float64)        # [iter, wave, 10]
    s = s_all[:, :waves]
    role = (np.arange(waves) % wpg) // 4          # 0 step, 1 service (chaser half if svc = 2), 2 service (target half)
    cyc = s[:, :, 7] - s[:, :, 0]
    real = (s[:, :, 9] - s[:, :, 8]) * 10.0          # ns
    print(f"shader clock while the kernel runs: {np.median(cyc / real):.2f} GHz (median over waves)")
    t0 = s[:, :, 8].min(axis=1, keepdims=True)
    names = ["step waves", "service waves" if svc == 1 else "service waves (chaser half)", "service waves (target half)"]
    for name, sel in [(names[k], role == k) for k in range(1 + svc)]:
        x = s[:, sel, :]
        d = np.diff(x[:, :, :8], axis=2)
        ent = (x[:, :, 8] - t0) * 10.0
        ext = (x[:, :, 9] - t0) * 10.0
        print(f"{name}: median cycles per phase 0>1>..>7 {np.median(d, axis=(0, 1)).astype(int).tolist()} | wave lifetime "
              f"{np.median(real[:, sel]):.0f} ns | enters {np.median(ent):.0f} ns (p95 {np.percentile(ent, 95):.0f}) and leaves "
              f"{np.median(ext):.0f} ns (p95 {np.percentile(ext, 95):.0f}, max {np.median(ext.max(axis=1)):.0f}) after the first wave")
    if target_form:
        at_join, wait_join = s[:, :, 2] - s[:, :, 0], s[:, :, 3] - s[:, :, 2]
        print("cycles from entry to the join, median by role: " + ", ".join(f"{names[k]} {np.median(at_join[:, role == k]):.0f}" for k in range(1 + svc))
              + " | waited at the join: " + ", ".join(f"{names[k]} {np.median(wait_join[:, role == k]):.0f}" for k in range(1 + svc)))
    at_barrier = s[:, :, k_barrier] - s[:, :, 0]
    print("cycles from entry to the barrier, median by role: " + ", ".join(f"{names[k]} {np.median(at_barrier[:, role == k]):.0f}" for k in range(1 + svc))
          + " | waited at the barrier: " + ", ".join(f"{np.median((s[:, :, k_barrier + 1] - s[:, :, k_barrier])[:, role == k]):.0f}" for k in range(1 + svc)))
    refill = s_all[:, waves::wpg]                    # wave 0 of every refill workgroup (all zero in the speculative form)
    if refill[:, :, 9].max() > 0:
        ent, ext = (refill[:, :, 8] - t0) * 10.0, (refill[:, :, 9] - t0) * 10.0
        step_ext = (s[:, role == 0, 9] - t0) * 10.0
        print(f"refill waves: lifetime {np.median(ext - ent):.0f} ns (p95 {np.percentile(ext - ent, 95):.0f}) | enter {np.median(ent):.0f} ns (p95 {np.percentile(ent, 95):.0f}) and leave "
              f"{np.median(ext):.0f} ns (p95 {np.percentile(ext, 95):.0f}, max {np.median(ext.max(axis=1)):.0f}) after the first wave | the last step wave leaves at "
              f"{np.median(step_ext.max(axis=1)):.0f} ns, the last refill wave {np.median(ext.max(axis=1) - step_ext.max(axis=1)):+.0f} ns from it")
        print(f"launch span with the refill waves: {np.median((s_all[:, :, 9].max(axis=1) - s[:, :, 8].min(axis=1)) * 10):.0f} ns")
    print(f"launch span seen by the waves (first entry -> last exit): {np.median((s[:, :, 9].max(axis=1) - s[:, :, 8].min(axis=1)) * 10):.0f} ns")


if __name__ == "__main__":
    main()

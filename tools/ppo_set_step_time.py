#!/usr/bin/env python3
"""Time of the update half of a sweep's learner step on the device (rdv_ppo_set_adam_step, csrc/rdv_ppo_adam.h: gradient clip, Adam and the
repack of the members' forward blocks in two launches) against the PyTorch path of the same build: per-member clip_grad_norm_, one
torch.optim.Adam over all members' parameters, PolicySet.update_weights.  P in {1, 8, 64} members, n = 128 samples per member, the rollout
and the members of tools/ppo_set_grad_time.py.

    python tools/ppo_set_step_time.py [--out profiles/ppo_set_step_time.csv] [--commit ID]

Before anything is timed the two paths take one step from the same weights and gradients and are compared: both sides' parameters against
the float64 reference of tests/ppo_adam_reference.py within its bound, and the device side's blocks against the host packer's on the same
weights (byte for byte outside the six exp(log_std) floats).
Rows, in microseconds, median of 5 samples of ~50 ms after warm-up and the spread (max - min), the two sides sampled in turn:
  `kernels`  the device call alone replayed from a HIP graph (its two kernels; the PyTorch side has no such form: update_weights is not
             legal in a capture);
  `update`   clip + Adam + weight refresh on fixed gradients, eager, wall clock around a synchronise: PolicySet.adam_step on one side,
             clip_grad_norm_ per member + optimizer.step() + update_weights() on the other;
  `step`     the whole Python step of INTEGRATION.md both ways: ppo_grads (SB3's advantage normalisation included) and the update."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd import _native as N  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import PolicySet  # noqa: E402
from ppo_grad_time import alternate  # noqa: E402
from ppo_set_grad_time import DEV, ROWS_PER_MEMBER, eager, members, rollout  # noqa: E402
import ppo_adam_reference as A  # noqa: E402

LR, EPS, MAX_NORM, N_SAMPLES = 1e-5, 1e-5, 0.5, 128


def flat_params(pset):
    """([P,5708], [P,5377]) float32 arrays of the member modules' parameters, the flat layout"""
    from reinforcement_learning_rendezvous_amd.ppo import _params
    rows = [[torch.cat([p.detach().reshape(-1) for p in part]).cpu().numpy() for part in _params(m)] for m in pset]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def blocks(pset):
    """[(block, is_actor)] of every member of both set handles"""
    return [(A.read_block(h, g), actor) for actor, h in ((True, pset._hip_handle(DEV)), (False, pset._critic_handle(DEV))) for g in range(len(pset))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_set_step_time.csv"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mlp_policy.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_set_step_time.py: no GPU: nothing is measured")
    command = "python tools/ppo_set_step_time.py " + " ".join(sys.argv[1:])
    rows = ["what,members,n_per_member,device_us,device_spread_us,torch_us,torch_spread_us,torch_over_device,worst_over_bound_device,worst_over_bound_torch,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(line):
        rows.append(line + f",{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")

    for P in [int(x) for x in args.members.split(",")]:
        gen = torch.Generator(device=DEV).manual_seed(P)
        dset = PolicySet(members(args.checkpoint, P), [ROWS_PER_MEMBER] * P)       # the device path
        tset = PolicySet(members(args.checkpoint, P), [ROWS_PER_MEMBER] * P)       # the PyTorch path, the same weights
        buf = rollout(dset.policies, gen)
        idx = [g * ROWS_PER_MEMBER + torch.randperm(ROWS_PER_MEMBER, device=DEV, generator=gen)[:N_SAMPLES] for g in range(P)]
        opt = torch.optim.Adam([p for m in tset for p in m.parameters()], lr=LR, eps=EPS)
        grads = lambda s: s.ppo_grads(buf, idx, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, check=False)

        def torch_update():
            for m in tset:
                torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM)
            opt.step()
            tset.update_weights()

        def device_update():
            dset.adam_step(None, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        # ---- one step on both sides from the same weights, compared before anything is timed
        pa0, pc0 = flat_params(dset)
        grads(dset); grads(tset)
        st = dset._ppo[torch.device(DEV)]
        ga, gc = st["actor"].cpu().numpy().copy(), st["critic"].cpu().numpy().copy()
        device_update(); torch_update()
        torch.cuda.synchronize()
        worst = []
        for s in (dset, tset):
            pa, pc = flat_params(s)
            w = 0.0
            for g in range(P):
                ref = A.Reference64(pa0[g], pc0[g], LR, (0.9, 0.999), EPS, MAX_NORM)
                ref.step(ga[g], gc[g])
                w = max(w, ref.worst(pa[g], pc[g]))
            worst.append(w)
        if worst[0] > 1.0:                                              # (the PyTorch side's figure is reported, not judged: it is the baseline)
            sys.exit(f"ppo_set_step_time.py: P = {P}: the device step leaves the float64 reference's bound: {worst[0]:.3f} (PyTorch's float32 step: {worst[1]:.3f})")
        packed_on_device = blocks(dset)
        dset.update_weights()                                           # the host packer on the same weights
        torch.cuda.synchronize()
        for (got, actor), (want, _) in zip(packed_on_device, blocks(dset)):
            msg = A.blocks_equal(got, want, actor)
            if msg:
                sys.exit(f"ppo_set_step_time.py: P = {P}: a block packed on the device differs from the host packer's: {msg}")
        bound = f"{worst[0]:.3f},{worst[1]:.3f}"

        # ---- the device call's kernels alone
        ad = dset._adam[torch.device(DEV)]
        a, c = dset._hip_handle(DEV), dset._critic_handle(DEV)
        mask = C.c_uint64((1 << P) - 1)

        def kernels():
            N.check(N.lib().rdv_ppo_set_adam_step(a, c, C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()), C.c_void_p(st["critic"].data_ptr()), mask,
                                                  LR, 0.9, 0.999, EPS, MAX_NORM, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        k, = alternate([kernels])
        emit(f"kernels,{P},{N_SAMPLES},{f(k)},,,,{bound}")
        d, t = eager([device_update, torch_update])
        emit(f"update,{P},{N_SAMPLES},{f(d)},{f(t)},{t[0] / d[0]:.2f},{bound}")

        def device_step():
            dset.adam_step(grads(dset), lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        def torch_step():
            grads(tset)
            torch_update()
        d, t = eager([device_step, torch_step])
        emit(f"step,{P},{N_SAMPLES},{f(d)},{f(t)},{t[0] / d[0]:.2f},{bound}")
        dset.close(); tset.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of a sweep's learner step for policy sets of other architectures than the shipped one: the two set calls —
rdv_ppo_mlp_set_loss_grad (csrc/rdv_ppo_mlp.h "the set form": P members' minibatches in four launches) and rdv_ppo_mlp_set_adam_step
(csrc/rdv_ppo_adam.h "every MLP architecture": clip, Adam and the repack of the members' forward blocks in two launches) — against the
path such a set took before there were any, built from the same commit: ppo_grad member by member, clip_grad_norm_ per member, one
torch.optim.Adam over all members' parameters, PolicySet.update_weights().  Architectures [32, 32] ReLU (custom/custom_networks.py) and
[64] x 4 tanh (the largest block), P = 8 members, n = 128 samples per member, drawn by a permutation from each member's 4,096 env columns
of a one-step rollout (tools/ppo_set_grad_time.py).  The members are the dense random nets of tests/ppo_mlp_set_helpers.py.

    python tools/ppo_mlp_set_step_time.py [--out profiles/ppo_mlp_set_step_time.csv] [--commit ID]

The columns are those of profiles/ppo_set_step_time.csv (`what` carries the architecture); `device` is the set calls' side, `torch` the
member-by-member path.  Before anything is timed the two sides' gradients are compared bit for bit, and both take one step from the same
weights and gradients: the parameters of both against the float64 step of tests/ppo_adam_reference.py within its bound
(worst_over_bound, at most 1), and the device side's blocks against the host packer's on the same weights (byte for byte outside the six
exp(log_std) floats).  Rows, in microseconds, median of 5 samples of ~50 ms after warm-up and the spread (max - min), the two sides
sampled in turn:
  `grads`    the gradient calls alone (no normalisation) replayed from a HIP graph: one rdv_ppo_mlp_set_loss_grad against P
             rdv_ppo_mlp_loss_grad on stand-alone handles, back to back on one stream;
  `kernels`  rdv_ppo_mlp_set_adam_step alone replayed from a HIP graph (its two kernels; the PyTorch side has no such form);
  `update`   clip + Adam + weight refresh on fixed gradients, eager, wall clock around a synchronise: PolicySet.adam_step against
             clip_grad_norm_ per member + optimizer.step() + update_weights();
  `step`     the whole Python step of INTEGRATION.md both ways: ppo_grads + adam_step against ppo_grad member by member and the PyTorch
             update."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd import _native as N  # noqa: E402
from reinforcement_learning_rendezvous_amd import ppo  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import PolicySet  # noqa: E402
from ppo_grad_time import alternate  # noqa: E402
from ppo_set_grad_time import DEV, ROWS_PER_MEMBER, eager, rollout  # noqa: E402
import numpy as np  # noqa: E402
import ppo_adam_reference as A  # noqa: E402
import ppo_mlp_set_helpers as H  # noqa: E402

ARCHS = [((32, 32), (32, 32), "relu"), ((64, 64, 64, 64), (64, 64, 64, 64), "tanh")]
P, N_SAMPLES, LR, EPS, MAX_NORM = 8, 128, 1e-5, 1e-5, 0.5


def c_calls(pair, pset, pols, buf, idx):
    """(set call, P stand-alone calls) as functions that enqueue on the current stream, and their output tensors"""
    lib, n = N.lib(), N_SAMPLES
    sa, sc = H.specs(pair)
    ga, gc = int(lib.rdv_ppo_mlp_grad_floats(C.byref(sa), 1)), int(lib.rdv_ppo_mlp_grad_floats(C.byref(sc), 0))
    stream = lambda: C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ptr = lambda k: buf[k].data_ptr()
    counts = (C.c_int64 * P)(*[n] * P)
    cat = torch.cat(idx)
    ws = torch.empty(int(lib.rdv_ppo_mlp_set_workspace_bytes(C.byref(sa), C.byref(sc), P, counts)), dtype=torch.uint8, device=DEV)
    outs = [torch.zeros(s, device=DEV) for s in ((P, ga), (P, gc), (P, N.PPO_SCALARS))]
    rows = N.PpoRows(ptr("obs"), ptr("actions"), ptr("log_prob"), ptr("advantages"), ptr("returns"), cat.data_ptr(), buf["obs"].shape[1])
    so = N.PpoSetOut(outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, None)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)

    def set_side():
        N.check(lib.rdv_ppo_mlp_set_loss_grad(a, c, C.byref(rows), counts, 0.2, 0.0, 0.5, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(so), stream()))

    alone_outs = [torch.zeros_like(t) for t in outs]
    wss = [torch.empty(int(lib.rdv_ppo_mlp_workspace_bytes(C.byref(sa), C.byref(sc), n)), dtype=torch.uint8, device=DEV) for _ in range(P)]
    per = [(p._hip_handle(DEV), p._critic_handle(DEV),
            N.PpoRows(ptr("obs"), ptr("actions"), ptr("log_prob"), ptr("advantages"), ptr("returns"), idx[g].data_ptr(), buf["obs"].shape[1]),
            N.PpoOut(alone_outs[0][g].data_ptr(), alone_outs[1][g].data_ptr(), alone_outs[2][g].data_ptr(), None, None)) for g, p in enumerate(pols)]

    def alone_side():
        for g, (ha, hc, r, o) in enumerate(per):
            N.check(lib.rdv_ppo_mlp_loss_grad(ha, hc, C.byref(r), n, 0.2, 0.0, 0.5, C.c_void_p(wss[g].data_ptr()), wss[g].numel(), C.byref(o), stream()))

    set_side.indices = cat          # RdvPpoRows holds its address only: the tensor must live as long as the function is called
    return set_side, alone_side, outs, alone_outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_mlp_set_step_time.csv"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_mlp_set_step_time.py: no GPU: nothing is measured")
    command = "python tools/ppo_mlp_set_step_time.py " + " ".join(sys.argv[1:])
    rows = ["what,members,n_per_member,device_us,device_spread_us,torch_us,torch_spread_us,torch_over_device,worst_over_bound_device,worst_over_bound_torch,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(line):
        rows.append(line + f",{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")

    for pair in ARCHS:
        name = "x".join(map(str, pair[0])) + "-" + pair[2]
        gen = torch.Generator(device=DEV).manual_seed(P)
        nets = H.member_nets(pair, P)
        pols = [H.policy_of(n).to(DEV) for n in nets]                           # stand-alone handles of the members' weights
        dset = PolicySet([H.policy_of(n).to(DEV) for n in nets], [ROWS_PER_MEMBER] * P)   # the set form
        tset = PolicySet([H.policy_of(n).to(DEV) for n in nets], [ROWS_PER_MEMBER] * P)   # the same set, its gradients member by member
        assert ppo.hip_set_route(dset) == "mlp"
        tset._hip_handle(DEV); tset._critic_handle(DEV)      # a learner loop's `collect` has made the set handles: update_weights refreshes them on both sides
        buf = rollout(pols, gen)
        idx = [g * ROWS_PER_MEMBER + torch.randperm(ROWS_PER_MEMBER, device=DEV, generator=gen)[:N_SAMPLES] for g in range(P)]
        set_side, alone_side, outs, alone_outs = c_calls(pair, dset, pols, buf, idx)
        set_side(); alone_side()
        torch.cuda.synchronize()
        if not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs, alone_outs)):
            sys.exit(f"ppo_mlp_set_step_time.py: {name}: the set call and the stand-alone calls differ")
        s, a = alternate([set_side, alone_side])
        emit(f"grads:{name},{P},{N_SAMPLES},{f(s)},{f(a)},{a[0] / s[0]:.2f},,")

        opt = torch.optim.Adam([p for m in tset for p in m.parameters()], lr=LR, eps=EPS)
        grads = lambda: dset.ppo_grads(buf, idx, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, check=False)

        def member_grads():
            for m, i in zip(tset, idx):
                m.ppo_grad(buf, i, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, check=False)

        def torch_update():
            for m in tset:
                torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM)
            opt.step()
            tset.update_weights()

        def device_update():
            dset.adam_step(None, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        # ---- one step on both sides from the same weights, compared before anything is timed
        flat = lambda x: [[torch.cat([p.detach().reshape(-1) for p in part]).cpu().numpy() for part in ppo._params(m)] for m in x]
        p0 = flat(dset)
        grads(); member_grads()
        torch.cuda.synchronize()
        for x, y in zip(dset, tset):
            if not all(torch.equal(p.grad, q.grad) for p, q in zip(x.parameters(), y.parameters())):
                sys.exit(f"ppo_mlp_set_step_time.py: {name}: PolicySet.ppo_grads and ppo_grad member by member differ")
        st = dset._ppo[torch.device(DEV)]
        ga, gc = st["actor"].cpu().numpy().copy(), st["critic"].cpu().numpy().copy()
        device_update(); torch_update()
        torch.cuda.synchronize()
        worst = []
        for x in (dset, tset):
            p1, w = flat(x), 0.0
            for g in range(P):
                z = [np.zeros_like(q, dtype=np.float64) for q in p0[g]]
                ref = A.step64(p0[g][0], p0[g][1], z[0], z[1], z[0], z[1], ga[g], gc[g], 0, LR, 0.9, 0.999, EPS, MAX_NORM)
                for k in range(2):
                    w = max(w, float((np.abs(p1[g][k].astype(np.float64) - ref[k]) / A.bound(ref[k], ref[6][k])).max()))
            worst.append(w)
        if worst[0] > 1.0:
            sys.exit(f"ppo_mlp_set_step_time.py: {name}: the device step leaves the float64 reference's bound: {worst[0]:.3f} (PyTorch's float32 step: {worst[1]:.3f})")

        blocks = lambda x: [A.read_block(h, g) for h in (x._hip_handle(DEV), x._critic_handle(DEV)) for g in range(P)]
        packed_on_device = blocks(dset)
        dset.update_weights()                                           # the host packer on the same weights
        torch.cuda.synchronize()
        for k, (got, want) in enumerate(zip(packed_on_device, blocks(dset))):
            msg = A.blocks_equal(got, want, k < P, A.MLP_STD)
            if msg:
                sys.exit(f"ppo_mlp_set_step_time.py: {name}: a block packed on the device differs from the host packer's (block {k}): {msg}")
        bound = f"{worst[0]:.3f},{worst[1]:.3f}"

        ad = dset._adam[torch.device(DEV)]
        ha, hc = dset._hip_handle(DEV), dset._critic_handle(DEV)
        mask = C.c_uint64((1 << P) - 1)

        def kernels():
            N.check(N.lib().rdv_ppo_mlp_set_adam_step(ha, hc, C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()), C.c_void_p(st["critic"].data_ptr()), mask,
                                                      LR, 0.9, 0.999, EPS, MAX_NORM, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        k, = alternate([kernels])
        emit(f"kernels:{name},{P},{N_SAMPLES},{f(k)},,,,{bound}")
        d, t = eager([device_update, torch_update])
        emit(f"update:{name},{P},{N_SAMPLES},{f(d)},{f(t)},{t[0] / d[0]:.2f},{bound}")

        def device_step():
            dset.adam_step(grads(), lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        def member_step():
            member_grads()
            torch_update()
        d, t = eager([device_step, member_step])
        emit(f"step:{name},{P},{N_SAMPLES},{f(d)},{f(t)},{t[0] / d[0]:.2f},{bound}")
        for x in (dset, tset, *pols):
            x.close()


if __name__ == "__main__":
    main()

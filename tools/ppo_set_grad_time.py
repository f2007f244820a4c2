#!/usr/bin/env python3
"""Time of the set form of the PPO minibatch gradients (rdv_ppo_set_loss_grad, csrc/rdv_ppo.h "the set form": P members' minibatches in
four launches) against what the library offers without it for the same result, built from the same commit: P calls of rdv_ppo_loss_grad
on stand-alone handles of the members' weights, back to back on one stream (4 P dependent launches).  P in {1, 8}, n in {128, 4,096}
samples per member, drawn by a permutation from each member's 4,096 env columns of a one-step rollout.

    python tools/ppo_set_grad_time.py [--out profiles/ppo_set_grad_time.csv] [--commit ID]

Rows `call`: the C calls alone (no normalisation), HIP-graph replay, the replay count chosen so that a sample lasts ~50 ms, the two sides
sampled in turn, the median of 5 samples each after warm-up and the spread (max - min), in microseconds per call (set side) or per P calls
(stand-alone side).  The outputs of the two sides are compared bit for bit before anything is timed.
Row `step` (P = 8, n = 128): the whole Python step of a learner loop on both sides — gradients (with SB3's advantage normalisation),
clip_grad_norm_ per member, Adam, update_weights — eager (update_weights is not legal in a capture), wall clock around a synchronise, the
same sampling; `call_share` is the set call's time of the `call` row over the set side's step."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd import _native as N  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy, PolicySet  # noqa: E402
from ppo_grad_time import SAMPLES, SAMPLE_MS, alternate  # noqa: E402

ROWS_PER_MEMBER = 4096
DEV = "cuda:0"


def members(checkpoint, P):
    """P policies with actor and critic: the checkpoint, each member's weights moved by its own small noise"""
    base = dict(np.load(checkpoint, allow_pickle=False))
    out = []
    for g in range(P):
        rng = np.random.default_rng([17, g])
        w = {k: (v + (0.02 * rng.standard_normal(v.shape)).astype(v.dtype) if g and v.dtype == np.float32 else v) for k, v in base.items()}
        out.append(MlpPolicy(w).to(DEV))
    return out


def rollout(pols, gen):
    """A one-step rollout [1, P * 4096, ...] whose member columns hold actions drawn from that member"""
    n = len(pols) * ROWS_PER_MEMBER
    obs = torch.rand((1, n, 17), device=DEV, generator=gen) * 2 - 1
    actions, log_prob, values = torch.empty((1, n, 6), device=DEV), torch.empty((1, n), device=DEV), torch.empty((1, n), device=DEV)
    with torch.no_grad():
        for g, p in enumerate(pols):
            sl = slice(g * ROWS_PER_MEMBER, (g + 1) * ROWS_PER_MEMBER)
            mean = p.mean(obs[0, sl])
            a = mean + torch.exp(p.log_std) * torch.randn((ROWS_PER_MEMBER, 6), device=DEV, generator=gen)
            actions[0, sl] = a
            log_prob[0, sl] = (-((a - mean) ** 2) / (2 * torch.exp(p.log_std) ** 2) - p.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
            values[0, sl] = p.value(obs[0, sl])
    return dict(obs=obs, actions=actions, log_prob=log_prob - (torch.rand((1, n), device=DEV, generator=gen) * 0.4 - 0.2),
                advantages=torch.randn((1, n), device=DEV, generator=gen), returns=values + torch.randn((1, n), device=DEV, generator=gen))


def c_calls(pset, pols, buf, idx):
    """(set call, P stand-alone calls) as functions that enqueue on the current stream, and their output tensors"""
    lib, P, n = N.lib(), len(pols), int(idx[0].numel())
    stream = lambda: C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ptr = lambda k: buf[k].data_ptr()
    counts = (C.c_int64 * P)(*[n] * P)
    cat = torch.cat(idx)
    ws = torch.empty(int(lib.rdv_ppo_set_workspace_bytes(P, counts)), dtype=torch.uint8, device=DEV)
    outs = [torch.zeros(s, device=DEV) for s in ((P, N.PPO_ACTOR_GRAD), (P, N.PPO_CRITIC_GRAD), (P, N.PPO_SCALARS))]
    rows = N.PpoRows(ptr("obs"), ptr("actions"), ptr("log_prob"), ptr("advantages"), ptr("returns"), cat.data_ptr(), buf["obs"].shape[1])
    so = N.PpoSetOut(outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, None)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)

    def set_side():
        N.check(lib.rdv_ppo_set_loss_grad(a, c, C.byref(rows), counts, 0.2, 0.0, 0.5, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(so), stream()))

    alone_outs = [torch.zeros_like(t) for t in outs]
    wss = [torch.empty(int(lib.rdv_ppo_workspace_bytes(n)), dtype=torch.uint8, device=DEV) for _ in range(P)]
    per = [(p._hip_handle(DEV), p._critic_handle(DEV),
            N.PpoRows(ptr("obs"), ptr("actions"), ptr("log_prob"), ptr("advantages"), ptr("returns"), idx[g].data_ptr(), buf["obs"].shape[1]),
            N.PpoOut(alone_outs[0][g].data_ptr(), alone_outs[1][g].data_ptr(), alone_outs[2][g].data_ptr(), None, None)) for g, p in enumerate(pols)]

    def alone_side():
        for g, (ha, hc, r, o) in enumerate(per):
            N.check(lib.rdv_ppo_loss_grad(ha, hc, C.byref(r), n, 0.2, 0.0, 0.5, C.c_void_p(wss[g].data_ptr()), wss[g].numel(), C.byref(o), stream()))

    set_side.indices = cat          # RdvPpoRows holds its address only: the tensor must live as long as the function is called
    return set_side, alone_side, outs, alone_outs


def eager(fs):
    """Median and spread (us per call) of each function's wall-clock samples of ~50 ms, the functions sampled in turn."""
    def once(f, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / reps
    for f in fs:
        once(f, 3)
    reps = [max(1, math.ceil(SAMPLE_MS * 1e3 / once(f, 3))) for f in fs]
    us = [[] for _ in fs]
    for _ in range(SAMPLES):
        for i, f in enumerate(fs):
            us[i].append(once(f, reps[i]))
    return [(statistics.median(u), max(u) - min(u)) for u in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_set_grad_time.csv"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mlp_policy.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_set_grad_time.py: no GPU: nothing is measured")
    command = "python tools/ppo_set_grad_time.py " + " ".join(sys.argv[1:])
    rows = ["what,members,n_per_member,set_us,set_spread_us,alone_us,alone_spread_us,alone_over_set,call_share,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(line):
        rows.append(line + f",{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")

    for P in (1, 8):
        gen = torch.Generator(device=DEV).manual_seed(P)
        pols = members(args.checkpoint, P)                      # the set's members, and the stand-alone learners (their own handles)
        twins = members(args.checkpoint, P)
        pset = PolicySet(twins, [ROWS_PER_MEMBER] * P)
        buf = rollout(pols, gen)
        call_us, idx128 = None, None
        for n in (128, 4096):
            idx = [g * ROWS_PER_MEMBER + torch.randperm(ROWS_PER_MEMBER, device=DEV, generator=gen)[:n] for g in range(P)]
            set_side, alone_side, outs, alone_outs = c_calls(pset, pols, buf, idx)
            set_side(); alone_side()
            torch.cuda.synchronize()
            if not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs, alone_outs)):
                sys.exit(f"ppo_set_grad_time.py: P = {P}, n = {n}: the set call and the stand-alone calls differ")
            s, a = alternate([set_side, alone_side])
            emit(f"call,{P},{n},{f(s)},{f(a)},{a[0] / s[0]:.2f},")
            if n == 128:
                call_us, idx128 = s[0], idx
        if P == 8:                                              # last: the steps move the weights of the two sides apart
            opt = torch.optim.Adam([p for m in pset for p in m.parameters()], lr=1e-5)
            opts = [torch.optim.Adam(p.parameters(), lr=1e-5) for p in pols]

            def set_step():
                pset.ppo_grads(buf, idx128, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, check=False)
                for m in pset:
                    torch.nn.utils.clip_grad_norm_(m.parameters(), 0.5)
                opt.step()
                pset.update_weights()

            def alone_step():
                for p, o, i in zip(pols, opts, idx128):
                    p.ppo_grad(buf, i, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, check=False)
                    torch.nn.utils.clip_grad_norm_(p.parameters(), 0.5)
                    o.step()
                    p.update_weights()

            ss, aa = eager([set_step, alone_step])
            emit(f"step,{P},128,{f(ss)},{f(aa)},{aa[0] / ss[0]:.2f},{call_us / ss[0]:.3f}")
        pset.close()
        for p in pols:
            p.close()


if __name__ == "__main__":
    main()

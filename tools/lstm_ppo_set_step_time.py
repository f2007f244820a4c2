"""The whole update step of a recurrent sweep on the GPU: ``LstmPolicySet.ppo_sequence_grads`` + ``LstmPolicySet.sequence_adam_step`` (ONE
rdv_lstm_ppo_set_loss_grad and ONE rdv_lstm_ppo_set_adam_step: clip, Adam and the repack of every member's blocks on the device) against
the path of the commit before the device step existed — the same ``ppo_sequence_grads``, then per member ``clip_grad_norm_``, PyTorch's
Adam and ``update_weights(member=g)`` (a device-to-host copy of the member's parameters, the host packer, a staged upload) — on the same
GPU, the same [T, N] buffers, the same weights and columns -> profiles/lstm_ppo_set_step_time.csv.

Shapes: P = 8 members of 256 columns each (N = 2048), T = 128, trunk [64, 64], H in {32, 256}, B_g in {1, 32} columns per member.
Rows per shape, in microseconds, `device` the new path, `torch` the old one:
  `step`     ppo_sequence_grads + the optimiser step, wall clock around a synchronise (the old path's host work is part of what is compared);
  `update`   the optimiser step alone on fixed gradients, wall clock around a synchronise: sequence_adam_step against the three host steps;
  `kernels`  rdv_lstm_ppo_set_adam_step alone, replayed from a HIP graph, device events around the replay (its four launches; no `torch` side).
Per row: warm-up calls of both sides, then ``--reps`` rounds in which the sides alternate; the median, the minimum and the maximum of the
rounds and the ratio of the medians.  Before timing both sides take one step from the same weights and gradients and every member's
parameters are compared with the float64 step of tests/ppo_adam_reference.py (column ``worst_over_bound``: at most 1), and the device
side's blocks with the host packer's on the same weights (tests/ppo_lstm_adam_helpers.blocks_equal; column ``blocks``).

    python tools/lstm_ppo_set_step_time.py [--reps 7] [--out profiles/lstm_ppo_set_step_time.csv]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import policy_lstm_reference as L  # noqa: E402
import ppo_adam_reference as A  # noqa: E402
import ppo_lstm_adam_helpers as K  # noqa: E402
from reinforcement_learning_rendezvous_amd import _native as N  # noqa: E402
from reinforcement_learning_rendezvous_amd import ppo  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy, LstmPolicySet  # noqa: E402

DEV = "cuda:0"
P, T, GROUP = 8, 128, 256
SHAPES = [(H, B) for H in (32, 256) for B in (1, 32)]
LR, EPS, MAX_NORM = 1e-5, 1e-5, 0.5


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def rounds(fns, reps, warmup, timer=wall):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(timer(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_ppo_set_step_time.csv"))
    ap.add_argument("--shapes", default=None, help="H:B[,H:B...] instead of the table's shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_ppo_set_step_time: no GPU: nothing is measured")
    shapes = SHAPES if args.shapes is None else [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    N_ENVS = P * GROUP
    dev = torch.device(DEV)
    lines = ["what,H,trunk,T,P,B_per_member,device_median_us,device_min_us,device_max_us,torch_median_us,torch_min_us,torch_max_us,torch_over_device,"
             "worst_over_bound_device,worst_over_bound_torch,blocks,reps"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    kw = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)
    for H, B in shapes:
        nets = [(L.default_init(H, (64, 64), "tanh", seed=5 + g), L.critic_of(L.default_init(H, (64, 64), "tanh", seed=52 + g))) for g in range(P)]
        make = lambda: LstmPolicySet([LstmPolicy(L.weights_dict(a, c), activation_fn="tanh", n_rows=GROUP).to(DEV) for a, c in nets], [GROUP] * P)
        dset, tset = make(), make()
        rng = np.random.default_rng([7, H, B])
        t = lambda a: torch.from_numpy(a).to(DEV)
        f32 = lambda *s: t(rng.standard_normal(s).astype(np.float32))
        buf = dict(obs=t(rng.uniform(-1, 1, (T, N_ENVS, 17)).astype(np.float32)), actions=f32(T, N_ENVS, 6) * 0.5, log_prob=f32(T, N_ENVS) * 0.1 - 5.0,
                   advantages=f32(T, N_ENVS), returns=f32(T, N_ENVS), done=t((rng.uniform(size=(T, N_ENVS)) < 0.02).astype(np.uint8)),
                   lstm_state0=(f32(N_ENVS, H) * 0.3, f32(N_ENVS, H) * 0.3), lstm_critic_state0=(f32(N_ENVS, H) * 0.3, f32(N_ENVS, H) * 0.3))
        pieces = [t((rng.permutation(GROUP)[:B] + g * GROUP).astype(np.int64)) for g in range(P)]
        params = lambda m: [p for group in ppo._sequence_params(m) for p in group]
        for m in tset:
            for p in params(m):
                p.requires_grad_(True)
        opt = torch.optim.Adam([p for m in tset for p in params(m)], lr=LR, eps=EPS)
        d_grads = lambda: dset.ppo_sequence_grads(buf, pieces, check=False, **kw)
        t_grads = lambda: tset.ppo_sequence_grads(buf, pieces, check=False, **kw)

        def device_update():
            dset.sequence_adam_step(None, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        def torch_update():
            for g, m in enumerate(tset):
                torch.nn.utils.clip_grad_norm_(params(m), MAX_NORM)
            opt.step()
            for g in range(P):
                tset.update_weights(member=g)

        # ---- one step on both sides from the same weights and gradients, compared before anything is timed
        flat = lambda x: [[torch.cat([p.detach().reshape(-1) for p in part]).cpu().numpy() for part in ppo._sequence_params(m)] for m in x]
        p0 = flat(dset)
        d_grads(); t_grads()
        torch.cuda.synchronize()
        st = dset._ppo_seq[dev]
        if not all(torch.equal(p.grad, q.grad) for x, y in zip(dset, tset) for p, q in zip(params(x), params(y))):
            sys.exit("lstm_ppo_set_step_time: the two sets' gradients differ")
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
        read = lambda x: [A.read_block(x._handle(prefix, DEV), g) for prefix in ("l", "v") for g in range(P)]
        packed_on_device = read(dset)
        dset.update_weights()                                           # the host packer on the same weights
        torch.cuda.synchronize()
        msgs = [K.blocks_equal(got, want, k < P) for k, (got, want) in enumerate(zip(packed_on_device, read(dset)))]
        blocks = "equal" if not any(msgs) else "DIFFER: " + next(m for m in msgs if m).replace(",", ";")
        tail = f"{worst[0]:.3f},{worst[1]:.3f},{blocks},{args.reps}"
        row = lambda what, d, tt: emit(f"{what},{H},64-64,{T},{P},{B},{statistics.median(d):.0f},{min(d):.0f},{max(d):.0f}," +
                                       (f"{statistics.median(tt):.0f},{min(tt):.0f},{max(tt):.0f},{statistics.median(tt) / statistics.median(d):.2f}" if tt else ",,,") +
                                       "," + tail)

        def device_step():
            dset.sequence_adam_step(d_grads(), lr=LR, eps=EPS, max_grad_norm=MAX_NORM)

        def torch_step():
            t_grads()
            torch_update()

        d, tt = rounds([device_step, torch_step], args.reps, args.warmup)
        row("step", d, tt)
        d, tt = rounds([device_update, torch_update], args.reps, args.warmup)
        row("update", d, tt)

        ad = dset._adam[dev]
        ha, hc = dset._handle("l", DEV), dset._handle("v", DEV)
        mask = C.c_uint64((1 << P) - 1)

        def kernels():
            N.check(N.lib().rdv_lstm_ppo_set_adam_step(ha, hc, C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()), C.c_void_p(st["critic"].data_ptr()), mask,
                                                       LR, 0.9, 0.999, EPS, MAX_NORM, C.c_void_p(ad["workspace"].data_ptr()), ad["workspace"].numel(),
                                                       C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            kernels()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            kernels()

        def replay_us(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3
        d, = rounds([graph.replay], args.reps, args.warmup, timer=replay_us)
        row("kernels", d, None)
        for x in (dset, tset):
            for m in x:
                m.close()
            x.close()
        del buf, dset, tset, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""``LstmPolicySet.ppo_sequence_grads`` on the GPU: ONE rdv_lstm_ppo_set_loss_grad call for P = 8 members against the eight stand-alone
``LstmPolicy.ppo_sequence_grad`` calls (rdv_lstm_ppo_loss_grad) it replaces — the same GPU, the same [T, N] buffers, the same weights,
the same columns -> profiles/lstm_ppo_set_grad_time.csv.

Shapes: P = 8 members of 256 columns each (N = 2048), T = 128, trunk [64, 64], H in {32, 256}, B_g in {1, 32, 256} columns per member.
Per shape: warm-up calls of both paths (handles, LDS limits, allocator), then ``--reps`` rounds; a round times the set call and then the
eight stand-alone calls, each with device events around it on an otherwise idle stream, so the two paths alternate under the same
conditions.  Reported per path: the median, the minimum and the maximum of the rounds, in microseconds, and the ratio of the medians.
Before timing, every member's gradients of the set call are compared with its stand-alone call's by ``torch.equal`` (column ``equal``).

    python tools/lstm_ppo_set_grad_time.py [--reps 7] [--out profiles/lstm_ppo_set_grad_time.csv]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import policy_lstm_reference as L  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy, LstmPolicySet  # noqa: E402

DEV = "cuda:0"
P, T, GROUP = 8, 128, 256
SHAPES = [(H, B) for H in (32, 256) for B in (1, 32, 256)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_ppo_set_grad_time.csv"))
    ap.add_argument("--shapes", default=None, help="H:B[,H:B...] instead of the table's shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_ppo_set_grad_time: no GPU: nothing is measured")
    shapes = SHAPES if args.shapes is None else [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    N = P * GROUP
    lines = ["H,trunk,T,P,B_per_member,set_median_us,set_min_us,set_max_us,eight_calls_median_us,eight_calls_min_us,eight_calls_max_us,ratio_of_medians,equal,reps"]
    kw = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)
    for H, B in shapes:
        weights = [L.weights_dict(L.default_init(H, (64, 64), "tanh", seed=5 + g), L.critic_of(L.default_init(H, (64, 64), "tanh", seed=52 + g))) for g in range(P)]
        members = [LstmPolicy(w, activation_fn="tanh", n_rows=GROUP).to(DEV) for w in weights]
        twins = [LstmPolicy(w, activation_fn="tanh", n_rows=1).to(DEV) for w in weights]
        lset = LstmPolicySet(members, [GROUP] * P)
        rng = np.random.default_rng([7, H, B])
        t = lambda a: torch.from_numpy(a).to(DEV)
        f32 = lambda *s: t(rng.standard_normal(s).astype(np.float32))
        buf = dict(obs=t(rng.uniform(-1, 1, (T, N, 17)).astype(np.float32)), actions=f32(T, N, 6) * 0.5, log_prob=f32(T, N) * 0.1 - 5.0,
                   advantages=f32(T, N), returns=f32(T, N), done=t((rng.uniform(size=(T, N)) < 0.02).astype(np.uint8)),
                   lstm_state0=(f32(N, H) * 0.3, f32(N, H) * 0.3), lstm_critic_state0=(f32(N, H) * 0.3, f32(N, H) * 0.3))
        pieces = [t((rng.permutation(GROUP)[:B] + g * GROUP).astype(np.int64)) for g in range(P)]
        one = lambda: lset.ppo_sequence_grads(buf, pieces, check=False, **kw)

        def eight():
            for g in range(P):
                twins[g].ppo_sequence_grad(buf, pieces[g], check=False, **kw)

        for _ in range(args.warmup):
            one(); eight()
        torch.cuda.synchronize()
        dev = torch.device(DEV)
        st = lset._ppo_seq[dev]
        equal = all(torch.equal(st["actor"][g], twins[g]._ppo_seq[dev]["actor"]) and torch.equal(st["critic"][g], twins[g]._ppo_seq[dev]["critic"]) and
                    torch.equal(st["scalars"][g], twins[g]._ppo_seq[dev]["scalars"]) for g in range(P))
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(one))
            b.append(timed(eight))
        ma, mb = statistics.median(a), statistics.median(b)
        lines.append(f"{H},64-64,{T},{P},{B},{ma:.0f},{min(a):.0f},{max(a):.0f},{mb:.0f},{min(b):.0f},{max(b):.0f},{mb / ma:.2f},{'yes' if equal else 'NO'},{args.reps}")
        print(lines[-1], flush=True)
        for p in members + twins + [lset]:
            p.close()
        del buf, lset, members, twins
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

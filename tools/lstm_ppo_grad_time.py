"""``LstmPolicy.ppo_sequence_grad`` on the GPU: rdv_lstm_ppo_loss_grad against the policy's own PyTorch fallback (float32 autograd through
the modules over the T steps, ``backend="torch"``, same device, same buffers) -> profiles/lstm_ppo_grad_time.csv.

Shapes: H = 256, trunk [64, 64], T = 128, B in {1, 32, 256, 2048}; H = 32 at B = 256.  Per shape and path: warm-up calls (handles, LDS
limits, allocator, autograd's workspace), then ``--reps`` calls timed one by one with device events around the call on an otherwise idle
stream; the median and the minimum are reported, in microseconds.  The comparison is not tuned: both paths take the call as a user makes it.

    python tools/lstm_ppo_grad_time.py [--reps 7] [--out profiles/lstm_ppo_grad_time.csv]
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
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 128, 1), (256, 128, 32), (256, 128, 256), (256, 128, 2048), (32, 128, 256)]


def time_calls(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_ppo_grad_time.csv"))
    ap.add_argument("--shapes", default=None, help="H:T:B[,H:T:B...] instead of the table's shapes (e.g. under rocprofv3 --kernel-trace --stats for the per-phase split)")
    ap.add_argument("--paths", default="hip,torch")
    args = ap.parse_args()
    shapes = SHAPES if args.shapes is None else [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",")]
    lines = ["H,trunk,T,B,path,median_us,min_us,reps"]
    for H, T, B in shapes:
        net = L.default_init(H, (64, 64), "tanh")
        w = L.weights_dict(net, L.critic_of(L.default_init(H, (64, 64), "tanh", seed=52)))
        rng = np.random.default_rng([7, H, B])
        t = lambda a: torch.from_numpy(a).to(DEV)
        f32 = lambda *s: t(rng.standard_normal(s).astype(np.float32))
        buf = dict(obs=t(rng.uniform(-1, 1, (T, B, 17)).astype(np.float32)), actions=f32(T, B, 6) * 0.5, log_prob=f32(T, B) * 0.1 - 5.0,
                   advantages=f32(T, B), returns=f32(T, B), done=t((rng.uniform(size=(T, B)) < 0.02).astype(np.uint8)),
                   lstm_state0=(f32(B, H) * 0.3, f32(B, H) * 0.3), lstm_critic_state0=(f32(B, H) * 0.3, f32(B, H) * 0.3))
        row = {}
        for path, backend, warm, reps in (("hip", "auto", 3, args.reps), ("torch", "torch", 2, max(3, args.reps // 2))):
            if path not in args.paths.split(","):
                continue
            pol = LstmPolicy(w, activation_fn="tanh", n_rows=B, backend=backend).to(DEV)
            med, best = time_calls(lambda: pol.ppo_sequence_grad(buf, None, check=False), warm, reps)
            pol.close()
            row[path] = med
            lines.append(f"{H},64x64,{T},{B},{path},{med:.1f},{best:.1f},{reps}")
            print(lines[-1], flush=True)
        if len(row) == 2:
            print(f"  H={H} T={T} B={B}: torch / hip = {row['torch'] / row['hip']:.2f}", flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

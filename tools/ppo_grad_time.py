#!/usr/bin/env python3
"""Time of MlpPolicy.ppo_grad on the HIP path (rdv_ppo_loss_grad, csrc/rdv_ppo.h: four launches) against what the library offered before
it for the same result: the fallback's forward + backward through autograd over the same modules on the same device.  Minibatch sizes
n = 128, 4,096 and 65,536 rows, drawn by a permutation from a rollout of that many rows, with SB3's advantage normalisation (torch, both
sides) and without it (the library call alone against forward + backward alone).

    python tools/ppo_grad_time.py [--out profiles/ppo_grad_time.csv] [--commit ID] [--sizes 128,4096,65536]

Each figure: HIP-graph replay of one call, the replay count chosen so that a sample lasts ~50 ms, the two sides sampled in turn, the median
of 5 samples each after warm-up and the spread (max - min), in microseconds per call.  The gradients of the two sides are compared at
every size timed (largest difference over largest gradient of a tensor, for the actor's and the critic's tensors)."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy  # noqa: E402
from reinforcement_learning_rendezvous_amd.ppo import ppo_minibatches  # noqa: E402

SAMPLES, SAMPLE_MS = 5, 50.0


def capture(f):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f()
    g.replay()
    torch.cuda.synchronize()
    return g


def once(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / replays


def alternate(fs):
    """Median and spread (us per call) of each function's samples, the functions sampled in turn."""
    graphs = [capture(f) for f in fs]
    replays = [max(1, min(4096, math.ceil(SAMPLE_MS * 1e3 / once(g, 1)))) for g in graphs]
    us = [[] for _ in fs]
    for _ in range(SAMPLES):
        for i, g in enumerate(graphs):
            us[i].append(once(g, replays[i]))
    return [(statistics.median(u), max(u) - min(u)) for u in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_grad_time.csv"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--sizes", default="128,4096,65536")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mlp_policy.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_grad_time.py: no GPU: nothing is measured")
    dev = "cuda:0"
    hip, ref = MlpPolicy.from_npz(args.checkpoint).to(dev), MlpPolicy.from_npz(args.checkpoint, backend="torch").to(dev)
    command = "python tools/ppo_grad_time.py " + " ".join(sys.argv[1:])
    rows = ["what,n,normalize_advantage,hip_us,hip_spread_us,torch_us,torch_spread_us,torch_over_hip,actor_grad_difference,critic_grad_difference,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for n in [int(x) for x in args.sizes.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(n)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
        obs = torch.rand((1, n, 17), device=dev, generator=gen) * 2 - 1
        with torch.no_grad():
            mean = ref.mean(obs.reshape(-1, 17)).reshape(1, n, 6)
            actions = mean + torch.exp(ref.log_std) * rnd(1, n, 6)
            log_prob = (-((actions - mean) ** 2) / (2 * torch.exp(ref.log_std) ** 2) - ref.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        buf = dict(obs=obs, actions=actions, log_prob=log_prob - (torch.rand((1, n), device=dev, generator=gen) * 0.4 - 0.2),
                   advantages=rnd(1, n), returns=ref.value(obs) + rnd(1, n))
        idx = ppo_minibatches(n, n, gen)[0]
        for norm in (True, False):
            fs = [lambda p=p: p.ppo_grad(buf, idx, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=norm, check=False) for p in (hip, ref)]
            for fn in fs:
                fn()
            torch.cuda.synchronize()
            diffs = [float((a.grad - b.grad).abs().max() / b.grad.abs().max()) for a, b in zip(hip.parameters(), ref.parameters())]
            names = [k for k, _ in hip.named_parameters()]
            diff = ",".join(f"{max(d for k, d in zip(names, diffs) if k.startswith(pre) or (pre == 'l' and k == 'log_std')):.2e}" for pre in ("l", "v"))
            h, t = alternate(fs)
            rows.append(f"ppo_grad,{n},{int(norm)},{f(h)},{f(t)},{t[0] / h[0]:.2f},{diff},{args.commit},\"{command}\"")
            print(rows[-1], flush=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(rows) + "\n")
    hip.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of MlpPolicy.ppo_grad of other architectures than the shipped one on the HIP path (rdv_ppo_mlp_loss_grad, csrc/rdv_ppo_mlp.h: four
launches) against what the library offered before it for these networks: ``ppo_grad(backend="torch")``, forward + backward through
autograd over the same modules on the same device.  Architectures [32, 32] ReLU, [64] x 4 tanh and [16] x 2 sigmoid; minibatch sizes
n = 128, 4,096 and 65,536 rows, drawn by a permutation from a rollout of that many rows, with SB3's advantage normalisation (torch, both
sides) and without it (the library call alone against forward + backward alone).

    python tools/ppo_mlp_grad_time.py [--out profiles/ppo_mlp_grad_time.csv] [--commit ID] [--sizes 128,4096,65536]

The method is that of tools/ppo_grad_time.py, whose functions this tool uses: HIP-graph replay of one call, the replay count chosen so
that a sample lasts ~50 ms, the two sides sampled in turn, the median of 5 samples each after warm-up and the spread (max - min), in
microseconds per call.  The gradients of the two sides are compared at every size timed."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from ppo_grad_time import alternate  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy  # noqa: E402
from reinforcement_learning_rendezvous_amd.ppo import ppo_minibatches  # noqa: E402

NETWORKS = (([32, 32], "relu"), ([64, 64, 64, 64], "tanh"), ([16, 16], "sigmoid"))


def weights_of(arch, act, seed=4):
    """SB3 state-dict keys of a freshly initialised actor and critic of ``arch`` (MlpPolicy(weights=None): orthogonal actor; the critic at
    PyTorch's initialisation), log_std = -0.7 (a learner's, not the initial zeros)."""
    p = MlpPolicy(weights=None, net_arch=arch, activation_fn=act, seed=seed)
    out = {"log_std": torch.full((6,), -0.7).numpy()}
    for trunk, head, prefix in (("policy_net", "action_net", "l"), ("value_net", "value_net", "v")):
        layers = p._layers(prefix)
        for l, lin in enumerate(layers[:-1]):
            out[f"mlp_extractor.{trunk}.{2 * l}.weight"], out[f"mlp_extractor.{trunk}.{2 * l}.bias"] = lin.weight.detach().numpy(), lin.bias.detach().numpy()
        out[f"{head}.weight"], out[f"{head}.bias"] = layers[-1].weight.detach().numpy(), layers[-1].bias.detach().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_mlp_grad_time.csv"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--sizes", default="128,4096,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_mlp_grad_time.py: no GPU: nothing is measured")
    dev = "cuda:0"
    command = "python tools/ppo_mlp_grad_time.py " + " ".join(sys.argv[1:])
    rows = ["net_arch,activation,n,normalize_advantage,hip_us,hip_spread_us,torch_us,torch_spread_us,torch_over_hip,actor_grad_difference,critic_grad_difference,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for arch, act in NETWORKS:
        w = weights_of(arch, act)
        hip, ref = MlpPolicy(w, activation_fn=act).to(dev), MlpPolicy(w, activation_fn=act, backend="torch").to(dev)
        for n in [int(x) for x in args.sizes.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(n)
            rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
            obs = torch.rand((1, n, 17), device=dev, generator=gen) * 2 - 1
            with torch.no_grad():
                mean = ref.mean(obs.reshape(-1, 17)).reshape(1, n, 6)
                actions = mean + torch.exp(ref.log_std) * rnd(1, n, 6)
                log_prob = (-((actions - mean) ** 2) / (2 * torch.exp(ref.log_std) ** 2) - ref.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
                returns = ref._value_torch(obs) + rnd(1, n)
            buf = dict(obs=obs, actions=actions, log_prob=log_prob - (torch.rand((1, n), device=dev, generator=gen) * 0.4 - 0.2),
                       advantages=rnd(1, n), returns=returns)
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
                rows.append(f"{'x'.join(str(w) for w in arch)},{act},{n},{int(norm)},{f(h)},{f(t)},{t[0] / h[0]:.2f},{diff},{args.commit},\"{command}\"")
                print(rows[-1], flush=True)
                with open(args.out, "w") as fh:
                    fh.write("\n".join(rows) + "\n")
        hip.close()


if __name__ == "__main__":
    main()

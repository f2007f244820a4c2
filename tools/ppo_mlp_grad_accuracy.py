#!/usr/bin/env python3
"""The accuracy table behind the bounds of tests/test_gpu_ppo_mlp_grad.py: for every pair of architectures and activation of
tests/ppo_mlp_reference.CASES, every shape (with and without an index vector; the 4 x 64 networks, whose workgroups own 128 rows, also at
127, 128 and 129), every gradient tensor and five scalars of rdv_ppo_mlp_loss_grad: err = max|G_gpu - G64| / max|G64| against the fp64
reference of tests/ppo_mlp_reference.py, e32 = the same quantity for PyTorch's float32 autograd of the same loss (CPU), and
err / max(e32, 2^-23).  One row per (architecture, activation, n, indexed, quantity).

    python tools/ppo_mlp_grad_accuracy.py [--out profiles/ppo_mlp_grad_accuracy.csv]

The last two lines printed are the largest ratio of a gradient tensor and of a scalar, and the bounds they yield: the smallest power of
two at least twice the ratio."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import ppo_mlp_reference as Q  # noqa: E402
import test_gpu_ppo_mlp_grad as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_mlp_grad_accuracy.csv"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_mlp_grad_accuracy.py: no GPU: nothing is measured")
    lines = ["actor_arch,critic_arch,activation,n,indexed,tensor,err,e32,err_over_max_e32_floor"]
    worst = {"grad": (0.0, ""), "scalar": (0.0, "")}
    for key in T.KEYS:
        pi, vf, act = key
        c, pol, cols = T.member(key)
        shapes = Q.SHAPES + (Q.SMALL_GROUP_SHAPES if key in T.FOUR_WAVES else ())
        top = {"grad": 0.0, "scalar": 0.0}
        for n in shapes:
            for indexed in (False, True):
                for name, err, e32 in T.measure(c, pol, cols, n, indexed)[0]:
                    ratio = err / max(e32, T.FLOOR)
                    kind = "grad" if "." in name else "scalar"
                    lines.append(f"{Q.M.arch_id(pi)},{Q.M.arch_id(vf)},{act},{n},{int(indexed)},{name},{err:.4e},{e32:.4e},{ratio:.4f}")
                    worst[kind] = max(worst[kind], (ratio, lines[-1]))
                    top[kind] = max(top[kind], ratio)
        print(f"{Q.case_id(key)}: largest ratio of a gradient tensor {top['grad']:.3f}, of a scalar {top['scalar']:.3f}", flush=True)
        pol.close()
        del T._MEMBERS[key]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    for kind in ("grad", "scalar"):
        ratio, row = worst[kind]
        print(f"largest ratio of a {kind}: {ratio:.4f} ({row}): C = {2.0 ** math.ceil(math.log2(2.0 * ratio)):g}")


if __name__ == "__main__":
    main()

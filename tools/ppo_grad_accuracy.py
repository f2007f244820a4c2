#!/usr/bin/env python3
"""The accuracy table behind the bound of tests/test_gpu_ppo_grad.py: for both members, every shape (with and without an index vector),
every one of the 13 gradient tensors and five scalars of rdv_ppo_loss_grad, err = max|G_gpu - G64| / max|G64| against the fp64 reference of
tests/ppo_reference.py, e32 = the same quantity for PyTorch's float32 autograd of the same loss (CPU), and err / max(e32, 2^-23).

    python tools/ppo_grad_accuracy.py [--out profiles/ppo_grad_accuracy.csv]

The last line printed is the largest ratio and the bound it yields: the smallest power of two at least twice it."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import ppo_reference as P  # noqa: E402
import test_gpu_ppo_grad as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_grad_accuracy.csv"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_grad_accuracy.py: no GPU: nothing is measured")
    lines, worst = ["member,n,indexed,tensor,err,e32,err_over_max_e32_floor"], (0.0, "")
    for member in sorted(P.MEMBERS):
        case = P.make_case(member)
        pol = T.make_policy(case["actor"], case["critic"])
        cols = {k: torch.from_numpy(case[k].copy()).to(T.DEV) for k in ("obs", "actions", "old_log_prob", "advantages", "returns")}
        for n in P.SHAPES:
            for indexed in (False, True):
                rows, _, _, _ = T.measure(case, pol, cols, n, indexed)
                for name, err, e32 in rows:
                    ratio = err / max(e32, T.FLOOR)
                    lines.append(f"{member},{n},{int(indexed)},{name},{err:.4e},{e32:.4e},{ratio:.4f}")
                    worst = max(worst, (ratio, lines[-1]))
        pol.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"largest ratio {worst[0]:.4f} ({worst[1]}): C = {2.0 ** math.ceil(math.log2(2.0 * worst[0])):g}")


if __name__ == "__main__":
    main()

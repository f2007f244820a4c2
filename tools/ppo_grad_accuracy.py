#!/usr/bin/env python3
"""The accuracy table behind the bound of tests/test_gpu_ppo_grad.py: for both members, every shape (with and without an index vector),
every one of the 13 gradient tensors and five scalars of rdv_ppo_loss_grad, err = max|G_gpu - G64| / max|G64| against the fp64 reference of
tests/ppo_reference.py, e32 = the same quantity for PyTorch's float32 autograd of the same loss (CPU), and err / max(e32, 2^-23).
Behind the seven small shapes come the large ones of the 65,536-row case: n = 4,096 and 65,536 with rows in order (indexed = 0) and
n = 1,048,576, the first 4,096 rows 256 times each, shuffled (indexed = 1), against the reference of the rows it repeats.

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
    for member in P.BASE_MEMBERS:
        case = P.make_case(member)
        pol = T.make_policy(case["actor"], case["critic"])
        shapes = [(n, indexed, T.measure(case, pol, T.device_columns(case), n, indexed)[0]) for n in P.SHAPES for indexed in (False, True)]
        big_cols = T.device_columns(P.big_case(member))
        for n in P.BIG_SHAPES + (P.REPEAT_BASE * P.REPEAT_TIMES,):
            rows, _, _, idx = T.measure_big(member, pol, big_cols, n)
            shapes.append((n, idx is not None, rows))
        for n, indexed, rows in shapes:
            for name, err, e32 in rows:
                ratio = err / max(e32, T.FLOOR)
                lines.append(f"{member},{n},{int(indexed)},{name},{err:.4e},{e32:.4e},{ratio:.4f}")
                worst = max(worst, (ratio, lines[-1]))
            grad = max(err / max(e32, T.FLOOR) for name, err, e32 in rows if "." in name)
            print(f"{member} n={n} indexed={int(indexed)}: largest ratio of a gradient tensor {grad:.3f}, of a scalar "
                  f"{max(err / max(e32, T.FLOOR) for name, err, e32 in rows if '.' not in name):.3f}")
        pol.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"largest ratio {worst[0]:.4f} ({worst[1]}): C = {2.0 ** math.ceil(math.log2(2.0 * worst[0])):g}")


if __name__ == "__main__":
    main()

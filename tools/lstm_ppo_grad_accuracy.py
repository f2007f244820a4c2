"""The accuracy table of rdv_lstm_ppo_loss_grad: every case of tests/ppo_lstm_reference.py (the cases of
tests/test_gpu_ppo_lstm_grad.py) on the GPU against the fp64 reference, beside PyTorch's float32 autograd ->
profiles/lstm_ppo_grad_accuracy.csv: case, H, T, B, tensor, err, e32, ratio = err / max(e32, 2^-23), C.

    python tools/lstm_ppo_grad_accuracy.py [--out profiles/lstm_ppo_grad_accuracy.csv]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import policy_lstm_reference as L  # noqa: E402
import ppo_lstm_reference as Q  # noqa: E402
from reinforcement_learning_rendezvous_amd import ppo  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_ppo_grad_accuracy.csv"))
    args = ap.parse_args()
    lines = ["case,H,T,B,tensor,err,e32,ratio,C"]
    worst = {Q.C_TENSOR: (0.0, ""), Q.C_SCALAR: (0.0, "")}
    for name in Q.CASES:
        case = Q.make_case(name)
        ref64, ref32 = Q.references(name)
        pol = LstmPolicy(L.weights_dict(case["actor"], case["critic"]), activation_fn=case["actor"]["act"], n_rows=case["N"]).to(DEV)
        t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        buf = dict(obs=t(case["obs"]), actions=t(case["actions"]), log_prob=t(case["old_log_prob"]), advantages=t(case["advantages"]),
                   returns=t(case["returns"]), done=t(case["done"]), lstm_state0=tuple(t(a) for a in case["actor_state0"]),
                   lstm_critic_state0=tuple(t(a) for a in case["critic_state0"]))
        envs = None if case["envs"] is None else t(case["envs"])
        res = pol.ppo_sequence_grad(buf, envs, clip_range=Q.EPS, ent_coef=Q.ENT, vf_coef=Q.VF, normalize_advantage=False)
        a, c = ppo._sequence_params(pol)
        got = [p.grad.detach().cpu().numpy().astype(np.float64) for p in a + c]
        for tensor, err, e32, C_ in Q.compare(Q.names(case["actor"], case["critic"]), got, {k: float(res[k]) for k in Q.SCALARS}, ref64, ref32):
            ratio = err / max(e32, Q.FLOOR)
            lines.append(f"{name},{case['H']},{case['T']},{case['B']},{tensor},{err:.4e},{e32:.4e},{ratio:.4f},{C_:g}")
            if ratio > worst[C_][0]:
                worst[C_] = (ratio, lines[-1])
        pol.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    for C_, (ratio, line) in worst.items():
        print(f"largest ratio under C = {C_:g}: {ratio:.4f}  ({line})")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of one step of the recurrent policy (csrc/rdv_policy_lstm.h: rdv_lstm_act / rdv_lstm_value, two launches each) per
lstm_hidden_size H in {32, 64, 128, 256} with the [64, 64] tanh trunk at n rows, beside what a user of main_rnn.py has today on the same
device: PyTorch fp32 torch.nn.LSTMCell + Linear layers of the same weights on the same rows, the state kept in place.

    python tools/lstm_time.py [--n 65536] [--out profiles/lstm_time.csv] [--commit ID]

Each figure: HIP-graph replay of 16 steps, 16 replays per sample between device events (256 steps), the two sides sampled in turn
(HIP, PyTorch, HIP, ...), the median of 5 samples each after warm-up and the spread (max - min), in microseconds per step.  Before
timing, both sides run 4 steps from the zero state on the rows timed and their actions, values and states are compared.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd import LstmPolicy  # noqa: E402

CALLS, REPLAYS, SAMPLES = 16, 16, 5


def capture(f):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def once(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (CALLS * REPLAYS)


def alternate(fs):
    graphs = [capture(f) for f in fs]
    us = [[] for _ in fs]
    for _ in range(SAMPLES):
        for i, g in enumerate(graphs):
            us[i].append(once(g))
    return [(statistics.median(u), max(u) - min(u)) for u in us]


class TorchSide:
    """LSTMCell + Linear modules holding the policy's weights; the state advances in place."""

    def __init__(self, pol, prefix, n, dev):
        H = pol.lstm_hidden_size
        lstm = pol._lstm(prefix)
        self.cell = torch.nn.LSTMCell(17, H).to(dev)
        with torch.no_grad():
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(self.cell, k).copy_(getattr(lstm, k + "_l0"))
        self.layers = [l.to(dev) for l in pol._layers(prefix)]
        self.actor = prefix == "l"
        self.h, self.c = torch.zeros((n, H), device=dev), torch.zeros((n, H), device=dev)

    @torch.no_grad()
    def step(self, obs):
        h, c = self.cell(obs, (self.h, self.c))
        self.h.copy_(h); self.c.copy_(c)
        x = h
        for lin in self.layers[:-1]:
            x = torch.tanh(lin(x))
        y = self.layers[-1](x)
        return torch.clamp(y, -1.0, 1.0) if self.actor else y[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_time.csv"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_time.py: no GPU: nothing is measured")
    dev, n = "cuda:0", args.n
    obs = (torch.rand((n, 17), device=dev) * 2 - 1).contiguous()
    out_a, out_v = torch.empty((n, 6), device=dev), torch.empty((n,), device=dev)
    command = "python tools/lstm_time.py " + " ".join(sys.argv[1:])
    rows = ["lstm_hidden_size,trunk,n,hip_act_us,hip_act_spread,hip_value_us,hip_value_spread,torch_act_us,torch_act_spread,"
            "torch_value_us,torch_value_spread,max_abs_diff_after_4_steps,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    for H in (32, 64, 128, 256):
        torch.manual_seed(H)
        pol = LstmPolicy(lstm_hidden_size=H, n_rows=n, backend="hip")
        ta, tv = TorchSide(pol, "l", n, dev), TorchSide(pol, "v", n, dev)
        diff = 0.0
        for _ in range(4):                                   # same results from both sides, at the size timed
            a, v = pol.act(obs, deterministic=True), pol.value(obs)
            diff = max(diff, float((a - ta.step(obs)).abs().max()), float((v - tv.step(obs)).abs().max()))
        diff = max(diff, float((pol.state[0] - ta.h).abs().max()), float((pol.critic_state[1] - tv.c).abs().max()))
        assert diff < 1e-4, (H, diff)
        ha, pa = alternate([lambda: pol.act(obs, deterministic=True, out=out_a), lambda: ta.step(obs)])
        hv, pv = alternate([lambda: pol.value(obs, out=out_v), lambda: tv.step(obs)])
        rows.append(f"{H},64-64 tanh,{n},{f(ha)},{f(hv)},{f(pa)},{f(pv)},{diff:.3g},{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        pol.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()

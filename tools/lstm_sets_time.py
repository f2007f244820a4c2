#!/usr/bin/env python3
"""Time of one step of a recurrent policy SET (include/rdv.h, "Recurrent policy sets": rdv_lstm_act / rdv_lstm_value on a set handle, one
cell launch and one trunk launch for all members) per lstm_hidden_size H in {32, 64, 128, 256} with the [64, 64] tanh trunk, beside what a
user had before sets: one stand-alone handle per member, called back to back on one stream (two launches per member; their kernels are
instruction-identical to the ones before sets, profiles/lstm_sets_isa_diff.md), and beside ONE network over all rows (a plain handle
of member 0's weights: what the set's call costs over a single block).  The workload: 65,536 rows as 8 members of 8,192.

    python tools/lstm_sets_time.py [--members 8] [--rows 8192] [--out profiles/lstm_sets_time.csv] [--commit ID]

The method of tools/lstm_time.py: HIP-graph replay of 16 steps, 16 replays per sample between device events (256 steps), the two sides
sampled in turn (set, stand-alone, one network, set, ...), the median of 5 samples each after warm-up and the spread (max - min), in
microseconds per step of ALL rows.  Before timing, both sides run 3 steps from the zero state on the rows timed and their actions, values and states are
compared by equality (the set's contract).  Every member has weights of its own: at H = 256 the 8 gate blocks are about 9 MiB behind
L2s of 4 MiB per XCD, where one stand-alone call streams one 1.1 MiB block.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from lstm_time import alternate  # noqa: E402
from reinforcement_learning_rendezvous_amd import LstmPolicy, LstmPolicySet  # noqa: E402


def members(H, P, n_rows=None):
    out = []
    for g in range(P):
        torch.manual_seed(1000 * H + g)
        out.append(LstmPolicy(lstm_hidden_size=H, n_rows=n_rows, backend="hip"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--rows", type=int, default=8192, help="rows per member (a multiple of 256)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_sets_time.csv"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_sets_time.py: no GPU: nothing is measured")
    dev, P, m = "cuda:0", args.members, args.rows
    n = P * m
    obs = (torch.rand((n, 17), device=dev) * 2 - 1).contiguous()
    parts = [obs[g * m:(g + 1) * m] for g in range(P)]                # contiguous row ranges, 16-byte aligned (m * 17 * 4 bytes apart)
    out_a, out_v = torch.empty((n, 6), device=dev), torch.empty((n,), device=dev)
    outs_a, outs_v = [out_a[g * m:(g + 1) * m] for g in range(P)], [out_v[g * m:(g + 1) * m] for g in range(P)]
    command = "python tools/lstm_sets_time.py " + " ".join(sys.argv[1:])
    rows = ["lstm_hidden_size,trunk,members,rows_per_member,set_act_us,set_act_spread,alone_act_us,alone_act_spread,act_set_over_alone,"
            "set_value_us,set_value_spread,alone_value_us,alone_value_spread,value_set_over_alone,one_net_act_us,one_net_act_spread,"
            "one_net_value_us,one_net_value_spread,equal_after_3_steps,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    for H in (32, 64, 128, 256):
        pset = LstmPolicySet(members(H, P), [m] * P, backend="hip")
        alone = members(H, P, n_rows=m)
        for g, p in enumerate(alone):
            p.noise_env_offset = g * m
        one = members(H, 1, n_rows=n)[0]
        one_a, one_v = torch.empty((n, 6), device=dev), torch.empty((n,), device=dev)

        def alone_act():
            for p, o, a in zip(alone, parts, outs_a):
                p.act(o, deterministic=True, out=a)

        def alone_value():
            for p, o, v in zip(alone, parts, outs_v):
                p.value(o, out=v)

        equal = True
        for _ in range(3):                                   # the same results from both sides, at the size timed
            a, v = pset.act(obs, deterministic=True).clone(), pset.value(obs).clone()
            alone_act(); alone_value()
            equal = equal and torch.equal(a, out_a) and torch.equal(v, out_v)
        equal = equal and torch.equal(pset.state[0], torch.cat([p.state[0] for p in alone])) \
            and torch.equal(pset.critic_state[1], torch.cat([p.critic_state[1] for p in alone]))
        assert equal, H
        sa, aa, oa = alternate([lambda: pset.act(obs, deterministic=True, out=out_a), alone_act, lambda: one.act(obs, deterministic=True, out=one_a)])
        sv, av, ov = alternate([lambda: pset.value(obs, out=out_v), alone_value, lambda: one.value(obs, out=one_v)])
        rows.append(f"{H},64-64 tanh,{P},{m},{f(sa)},{f(aa)},{sa[0] / aa[0]:.3f},{f(sv)},{f(av)},{sv[0] / av[0]:.3f},{f(oa)},{f(ov)},{equal},{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        pset.close()
        one.close()
        for p in alone:
            p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()

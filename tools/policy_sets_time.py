#!/usr/bin/env python3
"""Diagnostic: what one launch of a policy set costs, and what it saves (policy sets, include/rdv.h).

    python tools/policy_sets_time.py [--commit ID] [--out profiles/policy_sets_time.csv]

At 65,536 rows with P in {1, 8, 64} members, for the shipped 17-64-64 tanh architecture and [32, 32] ReLU, under HIP-graph replay:
  act      (a) the set's act   (b) ONE plain policy's act over all rows   (b') (b) again   (c) P stand-alone handles on their slices
  value    the same four over obs [16, n, 17] (the rows of a 16-step rollout)
  collect  (a) batch.collect(set, 16) on one ungrouped batch   (c) P batches of n / P envs, each with its own policy
The yardstick for (a) is (b), the existing kernel in the same run; the noise of the method is the (b) - (b') gap; (c) is what one
does without sets, and (c) / (a) the feature's gain.  The forms are sampled IN TURN, --repeats rounds over all of them; every figure is
the median of its replays with their minimum and maximum, in us per call.  A set reads P distinct parameter blocks instead of one
(P = 64, shipped block: 2.1 MB instead of 33 KB), so (a) may legitimately sit above (b)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
ARCHS = [("64-64", [64, 64], "tanh"), ("32-32", [32, 32], "relu")]
T_ROWS = 16


def _policies(arch, act, count):
    """`count` policies of one architecture with different weights (SB3's initialisation, seeds 0 ..), each with a critic"""
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    out = []
    for k in range(count):
        p = MlpPolicy(weights=None, net_arch=arch, activation_fn=act, seed=k)
        p.has_critic = True          # the critic trunk keeps PyTorch's initialisation: good enough for a timing
        out.append(p)
    return out


def _graph(fn, calls):
    """`fn` x `calls` back to back on one stream as a graph (after an eager warm-up, which makes the handles)"""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return g, calls


def _sample(g, calls, replays=4):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * calls)


def _in_turn(forms, repeats):
    """forms: {tag: (graph, calls)} -> {tag: (median, min, max)} with the forms sampled in turn"""
    out = {tag: [] for tag in forms}
    for _ in range(repeats):
        for tag, (g, calls) in forms.items():
            out[tag].append(_sample(g, calls))
    return {tag: (statistics.median(v), min(v), max(v)) for tag, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from reinforcement_learning_rendezvous_amd import PolicySet
    from reinforcement_learning_rendezvous_amd.batch import RendezvousBatch
    from reinforcement_learning_rendezvous_amd.params import make_params
    n = args.rows
    command = "python tools/policy_sets_time.py " + " ".join(sys.argv[1:])
    lines = ["arch,activation,rows,members,call,form,us_per_call_median,us_min,us_max,commit,command"]
    print(lines[0], flush=True)

    def emit(name, act, count, call, res):
        for tag, t in res.items():
            lines.append(f'{name},{act},{n},{count},{call},{tag},{t[0]:.3f},{t[1]:.3f},{t[2]:.3f},{args.commit},"{command.strip()}"')
            print(lines[-1], flush=True)

    gen = torch.Generator(device=DEV).manual_seed(1)
    obs = (torch.rand((n, 17), device=DEV, generator=gen) * 2 - 1).contiguous()
    obs_t = (torch.rand((T_ROWS, n, 17), device=DEV, generator=gen) * 2 - 1).contiguous()
    params = make_params(t_max=60.0)
    for name, arch, act in ARCHS:
        for count in [int(x) for x in args.members.split(",")]:
            m = n // count
            pset = PolicySet(_policies(arch, act, count), [m] * count)
            plain = _policies(arch, act, 1)[0]
            alone = _policies(arch, act, count)
            slices = pset.group_slices
            # ---- act
            out_a, out_b = torch.empty((n, 6), device=DEV), torch.empty((n, 6), device=DEV)
            out_c = torch.empty((n, 6), device=DEV)
            obs_c = [obs[s] for s in slices]                     # contiguous row ranges

            def act_c():
                for p, o, s in zip(alone, obs_c, slices):
                    p.act(o, deterministic=False, out=out_c[s], env_id_offset=s.start)
            calls = 64 if count <= 8 else 16
            forms = {"a_set": _graph(lambda: pset.act(obs, deterministic=False, out=out_a), calls),
                     "b_one_policy": _graph(lambda: plain.act(obs, deterministic=False, out=out_b), calls),
                     "b_one_policy_again": _graph(lambda: plain.act(obs, deterministic=False, out=out_b), calls),
                     "c_separate_handles": _graph(act_c, calls)}
            emit(name, act, count, "act", _in_turn(forms, args.repeats))
            del forms
            # ---- value over [16, n, 17]
            val_a, val_b = torch.empty((T_ROWS * n,), device=DEV), torch.empty((T_ROWS * n,), device=DEV)
            obs_tc = [obs_t[:, s, :].contiguous() for s in slices]   # each learner's own [16, m, 17] rows
            val_c = [torch.empty((T_ROWS * m,), device=DEV) for _ in slices]

            def value_c():
                for p, o, v in zip(alone, obs_tc, val_c):
                    p.value(o, out=v)
            calls = 16 if count <= 8 else 4
            forms = {"a_set": _graph(lambda: pset.value(obs_t, out=val_a), calls),
                     "b_one_policy": _graph(lambda: plain.value(obs_t, out=val_b), calls),
                     "b_one_policy_again": _graph(lambda: plain.value(obs_t, out=val_b), calls),
                     "c_separate_handles": _graph(value_c, calls)}
            emit(name, act, count, f"value[{T_ROWS}xN]", _in_turn(forms, args.repeats))
            del forms, obs_tc, val_c
            # ---- collect(.., 16): one batch and the set against P batches with their policies
            env = RendezvousBatch(n, params=params, device=DEV, seed=0)
            env.reset()
            parts = [RendezvousBatch(m, params=params, device=DEV, seed=0, env_id_offset=s.start) for s in slices]
            for e in parts:
                e.reset()
            bufs = {"a": None, "c": [None] * count}

            def collect_a():
                bufs["a"] = env.collect(pset, T_ROWS, out=bufs["a"])

            def collect_c():
                for k, (e, p) in enumerate(zip(parts, alone)):
                    bufs["c"][k] = e.collect(p, T_ROWS, out=bufs["c"][k])
            calls = 4 if count <= 8 else 1
            forms = {"a_set": _graph(collect_a, calls), "c_separate_handles": _graph(collect_c, calls)}
            emit(name, act, count, f"collect[{T_ROWS}]", _in_turn(forms, args.repeats))
            del forms, bufs
            env.close()
            for e in parts:
                e.close()
            for p in [pset, plain] + alone:
                p.close()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

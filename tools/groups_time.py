#!/usr/bin/env python3
"""Diagnostic: what one grouped launch costs, and what it saves (parameter groups, include/rdv.h).

    python tools/groups_time.py [--out profiles/groups_time.csv]

Under HIP-graph replay of back-to-back launches, as tools/n_sweep.py, at N = 65,536 and 524,288 envs with G in {1, 8, 64} it times
  (a) the grouped step of N envs in G groups (step_kernel_groups),
  (b) the ungrouped FUSED-variant step of the same N on the same build (step_kernel_parts): (a) - (b) is the cost of the indirection,
  (c) G separate ungrouped handles of N / G envs (variant auto) stepped back to back on one stream: what one does without groups;
      (c) / (a) is the feature's gain.
Every figure is the median of --repeats replays of the same graph, with their minimum and maximum: the spread of (b) is the
yardstick for (a) - (b)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _group_params(g_count):
    """G valid parameter sets that differ in what the kernels read (reward coefficients, KOZ radius, dt): a sensitivity grid."""
    from reinforcement_learning_rendezvous_amd.params import make_params
    return [make_params(koz_radius=3.0 + 2.0 * k / max(g_count - 1, 1), dt=(1.0, 0.5)[k % 2], t_max=60.0,
                        reward_kwargs=dict(collision_coef=0.5 + 0.01 * k, bonus_coef=8.0, fuel_coef=0.2, att_coef=1.0)) for k in range(g_count)]


def _time(envs, acts_of, steps, repeats):
    """us per timestep of stepping every batch of `envs` once per timestep, back to back on one stream, replayed from a graph"""
    import torch
    for t in range(8):
        for e in envs:
            e.step(acts_of(e, t))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(steps):
            for e in envs:
                e.step(acts_of(e, t))
    torch.cuda.synchronize()
    g.replay()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / (4 * steps))
    del g
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,524288")
    ap.add_argument("--groups", default="1,8,64")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from reinforcement_learning_rendezvous_amd.batch import RendezvousBatch
    lines = ["n_envs,groups,what,kernel,us_per_step_median,us_min,us_max"]
    print(lines[0], flush=True)

    def emit(n, g_count, what, kernel, t):
        lines.append(f"{n},{g_count},{what},{kernel},{t[0]:.3f},{t[1]:.3f},{t[2]:.3f}")
        print(lines[-1], flush=True)

    for n in [int(x) for x in args.sizes.split(",")]:
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        acts = [(torch.rand((n, 6), device="cuda:0", generator=gen) * 2 - 1).contiguous() for _ in range(4)]
        for g_count in [int(x) for x in args.groups.split(",")]:
            params, m = _group_params(g_count), n // g_count
            steps = 128 if g_count <= 8 else 32
            # (b) first and last: its own drift over the other two measurements is part of the yardstick
            for tag in ("b_ungrouped_fused", "a_grouped", "c_separate_handles", "b_ungrouped_fused_again"):
                if tag.startswith("b"):
                    envs = [RendezvousBatch(n, params=params[0], device="cuda:0", seed=0, variant="fused")]
                elif tag.startswith("a"):
                    envs = [RendezvousBatch(n, params=params, group_sizes=[m] * g_count, device="cuda:0", seed=0)]
                else:
                    envs = [RendezvousBatch(m, params=p, device="cuda:0", seed=0, env_id_offset=k * m) for k, p in enumerate(params)]
                views = {id(e): [a[k * m:(k + 1) * m] if len(envs) > 1 else a for a in acts] for k, e in enumerate(envs)}
                for e in envs:
                    e.reset()
                t = _time(envs, lambda e, step: views[id(e)][step % 4], steps, args.repeats)
                emit(n, g_count, tag, envs[0].last_kernel.replace(",", ";"), t)
                for e in envs:
                    e.close()
                del envs, views
                torch.cuda.empty_cache()
        del acts
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

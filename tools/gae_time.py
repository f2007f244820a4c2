#!/usr/bin/env python3
"""Time of rdv_gae (csrc/rdv_advantages.h) and of rdv_rollout_advantages end to end (two critic launches + the GAE kernel) against
what the library offered before them for the same result: `policy.value` on the rows plus a T-step PyTorch loop of the float32
expressions on the same device tensors (eleven small kernels per timestep).  Sizes (T, N): (64, 65,536), (512, 4,096) — the
latency-bound shape: 64 waves walking 512 rows each — and (64, 524,288).

    python tools/gae_time.py [--out profiles/gae_time.csv] [--commit ID] [--depths 2,4,8,16] [--sizes 64x65536,512x4096,64x524288]

rdv_gae is timed at each prefetch depth the kernel is instantiated for (RDV_GAE_DEPTH, read at the call; the library's default is
kGaeDepth) in turn with the PyTorch loop; the end-to-end pair at the default depth.  Each figure: HIP-graph replay, the replay count
chosen so that a sample lasts ~50 ms, the sides of a comparison sampled in turn, the median of 5 samples each after warm-up and the
spread (max - min), in microseconds per call.  For rdv_gae also the achieved bytes/s on the 17 algorithmic bytes per (t, env) — 4 + 1 + 4
read, 4 + 4 written — and its share of the 6.29 TB/s a float4 copy reaches on this chip.  The outputs of the two sides are compared
(torch.equal) at every size timed.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from reinforcement_learning_rendezvous_amd import gae  # noqa: E402
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy  # noqa: E402

SAMPLES, SAMPLE_MS = 5, 50.0
COPY_CEILING = 6.29e12          # bytes/s, float4 copy on an MI355X
BYTES_PER_ELEMENT = 17          # reward 4 + done 1 + values 4 read, advantages 4 + returns 4 written


def capture(f, calls):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def once(g, replays, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * replays)


def alternate(fs, calls):
    """Median and spread (us per call) of each function's samples, the functions sampled in turn; calls[i] calls per graph."""
    graphs = [capture(f, c) for f, c in zip(fs, calls)]
    replays = [max(1, min(256, math.ceil(SAMPLE_MS * 1e3 / (once(g, 1, c) * c)))) for g, c in zip(graphs, calls)]
    us = [[] for _ in fs]
    for _ in range(SAMPLES):
        for i, g in enumerate(graphs):
            us[i].append(once(g, replays[i], calls[i]))
    return [(statistics.median(u), max(u) - min(u)) for u in us]


def torch_loop(reward, done, values, last_value, g, c, one, advantages, returns):
    """The float32 sequence of include/rdv.h, one PyTorch operation per rounding, on device scalars made before the capture."""
    T = reward.shape[0]
    a = torch.zeros_like(last_value)
    for t in range(T - 1, -1, -1):
        nnt = one - done[t].to(torch.float32)
        nv = last_value if t == T - 1 else values[t + 1]
        delta = (reward[t] + (g * nv) * nnt) - values[t]
        a = delta + (c * nnt) * a
        advantages[t] = a
        torch.add(a, values[t], out=returns[t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gae_time.csv"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--depths", default="2,4,8,16")
    ap.add_argument("--sizes", default="64x65536,512x4096,64x524288")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mlp_policy.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gae_time.py: no GPU: nothing is measured")
    dev = "cuda:0"
    gamma, lam = 0.99, 0.95
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    g, c, one = f32(gamma), f32(gamma * lam), f32(1.0)
    pol = MlpPolicy.from_npz(args.checkpoint).to(dev)
    command = "python tools/gae_time.py " + " ".join(sys.argv[1:])
    rows = ["what,T,N,depth,us,spread_us,torch_us,torch_spread_us,torch_over_hip,bytes_per_s,share_of_copy_ceiling,commit,command"]
    f = lambda t: f"{t[0]:.2f},{t[1]:.2f}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(row):
        rows.append(row + f",{args.commit},\"{command}\"")
        print(rows[-1], flush=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")

    for size in args.sizes.split(","):
        T, n = (int(x) for x in size.split("x"))
        gen = torch.Generator(device=dev).manual_seed(T + n)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
        ro = dict(obs=(torch.rand((T, n, 17), device=dev, generator=gen) * 2 - 1), reward=rnd(T, n) * 10,
                  done=(torch.rand((T, n), device=dev, generator=gen) < 0.1).to(torch.uint8), last_obs=torch.rand((n, 17), device=dev, generator=gen) * 2 - 1)
        values, last_value = rnd(T, n) * 10, rnd(n) * 10
        adv, ret = torch.empty_like(values), torch.empty_like(values)
        adv_t, ret_t = torch.empty_like(values), torch.empty_like(values)
        loop = lambda: torch_loop(ro["reward"], ro["done"], values, last_value, g, c, one, adv_t, ret_t)
        loop()
        hip_calls = max(1, min(16, (1 << 22) // (T * n)))      # a few calls per graph while a call is short
        for depth in [int(d) for d in args.depths.split(",")]:
            os.environ["RDV_GAE_DEPTH"] = str(depth)
            kernel = lambda: gae(ro["reward"], ro["done"], values, last_value, gamma, lam, out=(adv, ret))
            adv.zero_(); ret.zero_()
            kernel()
            assert torch.equal(adv, adv_t) and torch.equal(ret, ret_t), (T, n, depth)
            h, t = alternate([kernel, loop], [hip_calls, 1])
            rate = BYTES_PER_ELEMENT * T * n / (h[0] * 1e-6)
            emit(f"rdv_gae,{T},{n},{depth},{f(h)},{f(t)},{t[0] / h[0]:.1f},{rate:.3e},{rate / COPY_CEILING:.3f}")
        del os.environ["RDV_GAE_DEPTH"]
        # end to end at the library's default depth: values of the rows, of last_obs, advantages and returns
        v_t, lv_t = torch.empty((T, n), device=dev), torch.empty((n,), device=dev)

        def baseline():
            pol.value(ro["obs"], out=v_t.reshape(-1))
            pol.value(ro["last_obs"], out=lv_t)
            torch_loop(ro["reward"], ro["done"], v_t, lv_t, g, c, one, adv_t, ret_t)
        baseline()
        pol.advantages(ro, gamma, lam)
        for k, want in (("values", v_t), ("last_value", lv_t), ("advantages", adv_t), ("returns", ret_t)):
            assert torch.equal(ro[k], want), (T, n, k)
        h, t = alternate([lambda: pol.advantages(ro, gamma, lam), baseline], [1, 1])
        emit(f"rdv_rollout_advantages,{T},{n},default,{f(h)},{f(t)},{t[0] / h[0]:.1f},,")
        del ro, values, adv, ret, adv_t, ret_t, v_t
        torch.cuda.empty_cache()
    pol.close()


if __name__ == "__main__":
    main()

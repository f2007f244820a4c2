"""
NumPy reference of generalised advantage estimation (include/rdv.h: rdv_gae): SB3's RolloutBuffer.compute_returns_and_advantage
written as SB3 writes it, on float32 arrays (`gae32`, what the kernel and `advantages.gae` must equal bit for bit) and on float64
arrays (`gae64`, the sanity check of the float32 loop), and the generators of the `done` patterns and inputs the tests use.
Runs on the CPU; no test in it.
"""
import numpy as np

SHAPES = [(1, 1), (2, 63), (7, 64), (33, 65), (48, 1000), (130, 257)]      # (T, N): T = 1, T below / above / no multiple of any prefetch
                                                                           # depth, N below, at and past a wave, ragged workgroups
PATTERNS = ("none", "all", "bernoulli", "last", "first")
DISCOUNTS = [(1.0, 1.0), (0.99, 0.95)]                                     # (gamma, gae_lambda)


def _gae(reward, done, values, last_value, gamma, gae_lambda, dt):
    """SB3's loop (stable_baselines3/common/buffers.py, RolloutBuffer.compute_returns_and_advantage).  There `dones` is the done row
    of the last step and episode_starts[t + 1] the done row of step t; both enter as float32 arrays, gamma and gae_lambda as Python
    floats."""
    rewards, values = np.asarray(reward, dtype=dt), np.asarray(values, dtype=dt)
    episode_starts_next = np.asarray(done).astype(dt)                      # row t: episode_starts[t + 1] (row T-1: `dones`)
    last_values = np.asarray(last_value, dtype=dt)
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    T = rewards.shape[0]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(T)):
        if step == T - 1:
            next_non_terminal = 1.0 - episode_starts_next[step]
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts_next[step]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    returns = advantages + values
    assert advantages.dtype == dt and returns.dtype == dt
    return advantages, returns


def gae32(reward, done, values, last_value, gamma, gae_lambda):
    with np.errstate(invalid="ignore", over="ignore"):
        return _gae(reward, done, values, last_value, gamma, gae_lambda, np.float32)


def gae64(reward, done, values, last_value, gamma, gae_lambda):
    return _gae(reward, done, values, last_value, gamma, gae_lambda, np.float64)


def done_pattern(name, T, n, rng):
    """uint8 [T,N]: no episode ends; every step ends one; Bernoulli(0.1); only the last step; only the first."""
    d = np.zeros((T, n), dtype=np.uint8)
    if name == "all":
        d[:] = 1
    elif name == "bernoulli":
        d[:] = rng.random((T, n)) < 0.1
    elif name == "last":
        d[T - 1] = 1
    elif name == "first":
        d[0] = 1
    else:
        assert name == "none", name
    return d


def inputs(T, n, pattern, seed=0):
    """(reward, done, values, last_value): rewards and values standard normal x 10, float32."""
    rng = np.random.default_rng([seed, T, n, PATTERNS.index(pattern)])
    f = lambda *shape: (rng.standard_normal(shape) * 10.0).astype(np.float32)
    return f(T, n), done_pattern(pattern, T, n, rng), f(T, n), f(n)


def all_cases():
    return [(T, n, pat, g, lam) for (T, n) in SHAPES for pat in PATTERNS for (g, lam) in DISCOUNTS]


def case_id(case):
    T, n, pat, g, lam = case
    return f"T{T}-N{n}-{pat}-g{g}-l{lam}"

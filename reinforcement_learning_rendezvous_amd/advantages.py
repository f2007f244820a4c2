"""
Generalised advantage estimation over the rows of a rollout: SB3's ``RolloutBuffer.compute_returns_and_advantage`` (called by
``collect_rollouts``; reference main.py:114) for all T steps at once.  CUDA tensors go to ONE HIP kernel (rdv_gae, csrc/rdv_advantages.h);
CPU tensors take a PyTorch restatement of the same float32 sequence.  Both are bit-identical to SB3's loop evaluated in NumPy float32
(include/rdv.h states the association; tests/advantages_reference.py restates the loop).

The reference never sets ``TimeLimit.truncated`` (vec_env.py:6-7), so SB3's time-limit bootstrap does not apply and is not built.
Advantage normalisation is SB3's ``train()``'s, per minibatch, and is not done here.
"""
import ctypes as C

import torch


def check_tensor(t, name, shape, dtype, device):
    """ValueError naming the tensor unless `t` is a contiguous tensor of this shape and dtype on this device."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.device == device and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}"
                         f"{'' if not isinstance(t, torch.Tensor) or t.is_contiguous() else ', not contiguous'}")


def check_discounts(gamma, gae_lambda):
    for name, x in (("gamma", gamma), ("gae_lambda", gae_lambda)):
        if not 0.0 <= float(x) <= 1.0:          # (False for NaN)
            raise ValueError(f"{name} must be in [0, 1] (got {x})")


def gae_torch(reward, done, values, last_value, gamma, gae_lambda, advantages, returns):
    """The float32 sequence of include/rdv.h in PyTorch operations, one rounding each (any device): g and c are float32 scalars, the
    product gamma * gae_lambda is taken in double and rounded once."""
    T = reward.shape[0]
    g = torch.tensor(float(gamma), dtype=torch.float32, device=reward.device)
    c = torch.tensor(float(gamma) * float(gae_lambda), dtype=torch.float32, device=reward.device)
    one = torch.tensor(1.0, dtype=torch.float32, device=reward.device)
    a = torch.zeros_like(last_value)
    for t in range(T - 1, -1, -1):
        nnt = one - done[t].to(torch.float32)
        nv = last_value if t == T - 1 else values[t + 1]
        delta = (reward[t] + (g * nv) * nnt) - values[t]
        a = delta + (c * nnt) * a
        advantages[t] = a
        returns[t] = a + values[t]
    return advantages, returns


def gae(reward, done, values, last_value, gamma=0.99, gae_lambda=0.95, out=None):
    """``(advantages, returns)`` [T,N] of ``reward`` [T,N] float32, ``done`` [T,N] uint8 (the row of step t: SB3's
    ``episode_starts[t+1]``), ``values`` [T,N] float32 and ``last_value`` [N] float32 — time-major and contiguous, as
    ``RendezvousBatch.rollout`` writes them.  The defaults are SB3's (main.py:39-48 sets neither).  ``out``: a pair of tensors to write
    into (they must not alias the inputs).  CUDA tensors: one kernel on the current stream; CPU tensors: the PyTorch restatement."""
    if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
        raise ValueError(f"reward: expected a [T,N] tensor, got {tuple(getattr(reward, 'shape', ()))}")
    (T, n), dev = reward.shape, reward.device
    if T <= 0 or n <= 0:
        raise ValueError(f"reward: T and N must be positive (got {(T, n)})")
    check_tensor(reward, "reward", (T, n), torch.float32, dev)
    check_tensor(done, "done", (T, n), torch.uint8, dev)
    check_tensor(values, "values", (T, n), torch.float32, dev)
    check_tensor(last_value, "last_value", (n,), torch.float32, dev)
    check_discounts(gamma, gae_lambda)
    if out is None:
        out = (torch.empty_like(reward), torch.empty_like(reward))
    advantages, returns = out
    check_tensor(advantages, "advantages", (T, n), torch.float32, dev)
    check_tensor(returns, "returns", (T, n), torch.float32, dev)
    if not reward.is_cuda:
        return gae_torch(reward, done, values, last_value, gamma, gae_lambda, advantages, returns)
    from . import _native as N
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    N.check(N.lib().rdv_gae(C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()), C.c_void_p(values.data_ptr()),
                            C.c_void_p(last_value.data_ptr()), T, n, float(gamma), float(gae_lambda),
                            C.c_void_p(advantages.data_ptr()), C.c_void_p(returns.data_ptr()), idx, stream))
    return advantages, returns

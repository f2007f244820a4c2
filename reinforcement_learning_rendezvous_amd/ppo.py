"""
The learner's step between ``RendezvousBatch.collect`` and ``optimizer.step()``: the loss of SB3's ``PPO.train()`` for one minibatch and
its gradients (stable_baselines3/ppo/ppo.py, the body of the ``for rollout_data in self.rollout_buffer.get(self.batch_size)`` loop, with
``clip_range_vf=None``; ``ActorCriticPolicy.evaluate_actions`` with a ``DiagGaussianDistribution``, common/distributions.py).

    for epoch in range(n_epochs):
        for idx in ppo_minibatches(T * N, batch_size, generator):
            stats = policy.ppo_grad(buf, idx, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)      # fills .grad, returns 0-dim tensors
            torch.nn.utils.clip_grad_norm_(policy.parameters(), 0.5)
            optimizer.step()
            policy.update_weights()

For CUDA rows the loss and the gradients are ONE call of the library: rdv_ppo_loss_grad for the shipped 17-64-64 tanh actor and critic
(include/rdv.h "PPO minibatch gradients"; csrc/rdv_ppo.h), rdv_ppo_mlp_loss_grad for every other architecture the GPU forward serves —
1..4 hidden layers of 16 / 32 / 64, tanh, ReLU or sigmoid, actor and critic of different shapes included ("PPO minibatch gradients for
every MLP architecture"; csrc/rdv_ppo_mlp.h): hand-written MFMA kernels on the current stream, no allocation, no synchronisation, legal
inside a stream capture.  CPU rows and ``backend="torch"`` run the same expressions through autograd over the policy's own modules and
fill the same ``.grad`` tensors; so does the one pair the library refuses, a 64-64 tanh net beside a net of another shape.  Gradient
clipping, the optimiser and its schedules are PyTorch's; ``update_weights`` repacks as it always did.

A sweep of P learners on one GPU (``PolicySet``, one grouped batch) takes the same step for all members at once:

    for epoch in range(n_epochs):
        for pieces in ppo_set_minibatches(learners, T, batch_size, generator):                # step k: one index tensor per member
            stats = learners.ppo_grads(buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
            for member in learners:
                torch.nn.utils.clip_grad_norm_(member.parameters(), 0.5)
            optimizer.step()                                                                  # one optimiser over all members' parameters
            learners.update_weights()

``PolicySet.ppo_grads`` is ONE call of rdv_ppo_set_loss_grad (include/rdv.h "PPO minibatch gradients for policy sets"): the members'
minibatches share four launches, and every member gets the bits of its own ``MlpPolicy.ppo_grad``.  A set of another architecture the
forward kernels serve takes ONE rdv_ppo_mlp_set_loss_grad in the same way ("PPO minibatch gradients for policy sets of every MLP
architecture"; ``hip_set_route``); and the same ``adam_step`` (rdv_ppo_mlp_set_adam_step).

The three lines behind it can stay on the device too (CUDA rows, every architecture the forward kernels serve):

    for epoch in range(n_epochs):
        for pieces in ppo_set_minibatches(learners, T, batch_size, generator):
            stepped = learners.ppo_grads(buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
            learners.adam_step(stepped, lr=3e-4, max_grad_norm=0.5)                           # clip, Adam and the new forward blocks

``PolicySet.adam_step`` is ONE call of rdv_ppo_set_adam_step (include/rdv.h "Gradient clip, Adam and weight repack for policy sets";
rdv_ppo_mlp_set_adam_step for a set of another architecture): the
joint gradient norm of each member's actor and critic, Adam on fp32 master weights the set owns (the member modules' parameters are views
of them), and the members' forward blocks repacked on the device: no ``update_weights``, no host copy, legal inside a stream capture.

A recurrent learner (``LstmPolicy``) takes ``ppo_sequence_grad`` on minibatches of whole env columns (rdv_lstm_ppo_loss_grad, include/rdv.h
"Recurrent PPO minibatch gradients"); a sweep of them (``LstmPolicySet``) takes ``ppo_sequence_grads`` for all members in ONE call of
rdv_lstm_ppo_set_loss_grad, every member with the bits of its own ``ppo_sequence_grad``:

    for pieces in ppo_sequence_set_minibatches(learners, envs_per_batch, generator):          # step k: one tensor of columns per member
        stats = learners.ppo_sequence_grads(buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
        for g, member in enumerate(learners):                                                 # clipping and the optimiser: PyTorch's
            if pieces[g] is not None:
                torch.nn.utils.clip_grad_norm_(member.parameters(), 0.5); optimizers[g].step(); learners.update_weights(member=g)
"""
import ctypes as C
import math

import torch

_LOG_2PI = math.log(2.0 * math.pi)
SCALAR_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")


def ppo_minibatches(n_rows, batch_size, generator=None, device=None):
    """The index tensors of one epoch over ``n_rows`` flat rollout rows: a ``torch.randperm`` on the device (the generator's, unless
    ``device`` says otherwise) cut into consecutive pieces of ``batch_size`` as SB3's ``RolloutBuffer.get`` cuts its permutation
    (common/buffers.py: ``indices[start_idx : start_idx + batch_size]``); the last one may be short.  Every row appears exactly once.
    The tensors are marked as in range for ``n_rows``, so ``ppo_grad`` does not check them again."""
    n_rows, batch_size = int(n_rows), int(batch_size)
    if n_rows <= 0 or batch_size <= 0:
        raise ValueError(f"ppo_minibatches: n_rows = {n_rows} and batch_size = {batch_size} must be positive")
    if device is None:
        device = generator.device if generator is not None else "cpu"
    perm = torch.randperm(n_rows, generator=generator, device=device)
    parts = list(torch.split(perm, batch_size))
    for p in parts:
        p._rdv_ppo_rows = n_rows
    return parts


def ppo_set_minibatches(pset, n_steps, batch_size, generator=None, device=None):
    """One epoch for all members of a ``PolicySet`` over a ``[T, N]`` rollout (T = ``n_steps``, N the set's rows): member g gets a
    ``torch.randperm(T * size_g)``, drawn in member order from the one generator and cut into pieces of ``batch_size`` as
    ``ppo_minibatches`` cuts; local row j of member g is the flat row ``(j // size_g) * N + start_g + j % size_g`` of the buffer (step
    j // size_g, the member's env column j % size_g).  Returns a list of steps; step k is a list of P int64 tensors of flat rows, ``None``
    for a member whose pieces have run out (unequal group sizes give unequal piece counts).  Over the epoch every member sees each of its
    T * size_g rows exactly once.  The tensors are marked as checked for this set and T, so ``PolicySet.ppo_grads`` does not check them
    again."""
    n_steps, batch_size = int(n_steps), int(batch_size)
    if n_steps <= 0 or batch_size <= 0:
        raise ValueError(f"ppo_set_minibatches: n_steps = {n_steps} and batch_size = {batch_size} must be positive")
    if device is None:
        device = generator.device if generator is not None else "cpu"
    N = int(pset.num_rows)
    per = []
    for sl in pset.group_slices:
        size = sl.stop - sl.start
        perm = torch.randperm(n_steps * size, generator=generator, device=device)
        flat = torch.div(perm, size, rounding_mode="floor") * N + (sl.start + perm % size)
        pieces = list(torch.split(flat, batch_size))
        for p in pieces:
            p._rdv_ppo_set = (n_steps * N, N, sl.start, sl.stop)
        per.append(pieces)
    return [[pieces[k] if k < len(pieces) else None for pieces in per] for k in range(max(len(pieces) for pieces in per))]


def ppo_loss_terms(mean, log_std, values, actions, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef):
    """SB3's expressions on torch tensors of any dtype: ``mean`` [n,6], ``values`` [n] of the current networks.  Returns (loss, dict of
    the six scalars, log_prob [n])."""
    var = torch.exp(log_std) ** 2
    log_prob = (-((actions - mean) ** 2) / (2 * var) - log_std - 0.5 * _LOG_2PI).sum(-1)        # Normal.log_prob, summed over the action
    entropy = (0.5 + 0.5 * _LOG_2PI + log_std).expand_as(mean).sum(-1)                          # Normal.entropy, summed
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = ((returns - values) ** 2).mean()                                                # F.mse_loss(returns, values_pred)
    entropy_loss = -entropy.mean()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        approx_kl = ((torch.exp(log_ratio) - 1) - log_ratio).mean()
        clip_fraction = (torch.abs(ratio - 1) > clip_range).to(ratio.dtype).mean()
    scalars = dict(loss=loss.detach(), policy_loss=policy_loss.detach(), value_loss=value_loss.detach(), entropy_loss=entropy_loss.detach(),
                   approx_kl=approx_kl, clip_fraction=clip_fraction)
    return loss, scalars, log_prob


def normalize_advantages(a):
    """SB3's expression (ppo.py: ``(advantages - advantages.mean()) / (advantages.std() + 1e-8)``), applied when the minibatch has more
    than one sample."""
    return (a - a.mean()) / (a.std() + 1e-8)


def _params(policy):
    """The 13 parameter tensors (any architecture: 2 per layer) in the order of the flat gradient buffers: actor layers, log_std, critic layers."""
    actor = [t for lin in policy._layers("l") for t in (lin.weight, lin.bias)] + [policy.log_std]
    critic = [t for lin in policy._layers("v") for t in (lin.weight, lin.bias)]
    return actor, critic


def _specs(policy):
    """(actor spec, critic spec) as RdvMlpSpec."""
    from . import _native as N
    from .policy import ACTIVATIONS
    act = ACTIVATIONS[policy.activation][0]
    return N.MlpSpec.make(policy.pi_arch, act), N.MlpSpec.make(policy.vf_arch, act)


def hip_route(policy):
    """Which library call serves ``ppo_grad`` of this policy on CUDA rows: "shipped" (rdv_ppo_loss_grad: both nets 17-64-64 tanh),
    "mlp" (rdv_ppo_mlp_loss_grad: both nets of another architecture the GPU forward serves) or None (autograd: a width or depth the
    forward kernels do not serve, or exactly one net of the shipped shape, the pair rdv_ppo_mlp_loss_grad refuses)."""
    if policy.l1.in_features != 17:
        return None
    served = lambda arch: 1 <= len(arch) <= 4 and all(w in (16, 32, 64) for w in arch)
    default = [arch == [64, 64] and policy.activation == "tanh" for arch in (policy.pi_arch, policy.vf_arch)]
    if all(default):
        return "shipped"
    if any(default) or not (served(policy.pi_arch) and served(policy.vf_arch)):
        return None
    return "mlp"


def hip_set_route(pset):
    """Which library call serves ``PolicySet.ppo_grads`` (and, behind it, ``adam_step``) of this set on CUDA rows: "shipped"
    (rdv_ppo_set_loss_grad), "mlp" (rdv_ppo_mlp_set_loss_grad: one spec per set, both nets of another architecture the GPU forward
    serves) or None (member by member): the rules of ``hip_route`` for the members' common architecture, plus ``backend != "torch"``
    and at most 64 members.  A shipped set of more than 64 members still answers "shipped": ``ppo_grads`` of such a set is refused by
    the library's own cap (ValueError), as it always was, and its ``adam_step`` is the PyTorch fallback."""
    if pset.backend == "torch":
        return None
    route = hip_route(pset.policies[0])
    if len(pset) > 64 and route == "mlp":
        return None
    return route


def _state(policy, dev, n, rows):
    """The buffers the policy owns for ppo_grad on device ``dev``: two flat gradient buffers (the parameters' ``.grad`` are views of them
    when the modules live on ``dev``), the scalars, and — HIP path — the workspace and the advantage column, grown when a call needs more."""
    st = policy.__dict__.setdefault("_ppo", {}).get(dev)
    actor, critic = _params(policy)
    if st is None:
        st = dict(actor=torch.zeros(sum(p.numel() for p in actor), dtype=torch.float32, device=dev),
                  critic=torch.zeros(sum(p.numel() for p in critic), dtype=torch.float32, device=dev),
                  scalars=torch.zeros(8, dtype=torch.float32, device=dev), workspace=None, adv=None, n=0)
        policy._ppo[dev] = st
    if n is not None and (st["workspace"] is None or st["n"] < n):
        from . import _native as N
        if hip_route(policy) == "mlp":
            a, c = _specs(policy)
            need = int(N.lib().rdv_ppo_mlp_workspace_bytes(C.byref(a), C.byref(c), n))
        else:
            need = int(N.lib().rdv_ppo_workspace_bytes(n))
        st["workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
        st["n"] = n
    if rows is not None and (st["adv"] is None or st["adv"].numel() < rows):
        st["adv"] = torch.zeros(rows, dtype=torch.float32, device=dev)
    return st


def _bind_grads(policy, st, dev, params=None):
    """``.grad`` of every parameter <- its piece of the flat buffers: a view when the parameter lives on ``dev``, a copy otherwise.
    ``params``: (actor list, critic list) in the buffers' order; None: ``_params(policy)``."""
    for flat, params in zip((st["actor"], st["critic"]), params or _params(policy)):
        at = 0
        for p in params:
            piece = flat[at:at + p.numel()].view(p.shape)
            at += p.numel()
            if p.device == piece.device:
                if p.grad is None or p.grad.data_ptr() != piece.data_ptr():
                    p.grad = piece
            else:
                if p.grad is None:
                    p.grad = torch.empty_like(p)
                p.grad.copy_(piece)


def _columns(buf):
    obs = buf["obs"]
    if not isinstance(obs, torch.Tensor) or obs.dim() < 2 or obs.shape[-1] != 17:
        raise ValueError(f"ppo_grad: buf['obs']: expected a [T,N,17] tensor, got {tuple(getattr(obs, 'shape', ()))}")
    rows, dev = obs.numel() // 17, obs.device
    cols = dict(obs=(17,), actions=(6,), log_prob=(), advantages=(), returns=())
    flat = {}
    for name, tail in cols.items():
        t = buf.get(name)
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != rows * (tail[0] if tail else 1):
            raise ValueError(f"ppo_grad: buf[{name!r}] must be a contiguous float32 tensor of {rows} rows on {dev} (what RendezvousBatch.collect returns)")
        flat[name] = t.view((rows,) + tail)                           # a view, not a copy
    return flat, rows, dev


def _check_coefficients(who, clip_range, ent_coef, vf_coef):
    for name, v, low in (("clip_range", clip_range, None), ("ent_coef", ent_coef, 0.0), ("vf_coef", vf_coef, 0.0)):
        v = float(v)
        if not math.isfinite(v) or (v <= 0.0 if low is None else v < low):
            raise ValueError(f"{who}: {name} = {v!r} must be finite and " + ("positive" if low is None else "not negative"))


def ppo_grad(policy, buf, indices=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
    """See ``MlpPolicy.ppo_grad``."""
    from .policy import MlpPolicy
    if not isinstance(policy, MlpPolicy):
        raise TypeError(f"ppo_grad: a {type(policy).__name__} is not offered: it serves one MlpPolicy (a PolicySet has ppo_grads for all "
                        "its members at once; LstmPolicy and LstmPolicySet keep SB3 / PyTorch for the update)")
    if not policy.has_critic:
        raise ValueError("ppo_grad: this policy has no critic (its weights hold no value_net trunk)")
    _check_coefficients("ppo_grad", clip_range, ent_coef, vf_coef)
    cols, rows, dev = _columns(buf)
    if indices is None:
        n = rows
    else:
        if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64 or indices.dim() != 1 or indices.device != dev or indices.numel() == 0:
            raise ValueError(f"ppo_grad: indices must be a non-empty 1-d int64 tensor on {dev}")
        indices = indices.contiguous()
        n = int(indices.numel())
        if check and getattr(indices, "_rdv_ppo_rows", None) != rows:
            lo, hi = (int(x) for x in torch.aminmax(indices))
            if lo < 0 or hi >= rows:
                raise IndexError(f"ppo_grad: indices span [{lo}, {hi}], the rollout has rows 0..{rows - 1}")
    route = hip_route(policy) if policy.backend != "torch" and dev.type == "cuda" else None
    hip = route is not None
    take = (lambda t: t[:n]) if indices is None else (lambda t: t[indices])
    adv = take(cols["advantages"])
    if normalize_advantage and n > 1:
        adv = normalize_advantages(adv)

    if not hip:
        pdev = policy.l1.weight.device
        st = _state(policy, pdev, None, None)
        actor, critic = _params(policy)
        params = actor + critic
        flags = [p.requires_grad for p in params]
        try:
            for p in params:
                p.requires_grad_(True)
            with torch.enable_grad():
                obs = take(cols["obs"]).to(pdev)
                mean, values = policy._forward("l", obs), policy._forward("v", obs).squeeze(-1)
                loss, scalars, _ = ppo_loss_terms(mean, policy.log_std, values, take(cols["actions"]).to(pdev), take(cols["log_prob"]).to(pdev),
                                                  adv.to(pdev), take(cols["returns"]).to(pdev), float(clip_range), float(ent_coef), float(vf_coef))
                grads = torch.autograd.grad(loss, params)
        finally:
            for p, f in zip(params, flags):
                p.requires_grad_(f)
        with torch.no_grad():
            torch.cat([g.reshape(-1) for g in grads[:len(actor)]], out=st["actor"])
            torch.cat([g.reshape(-1) for g in grads[len(actor):]], out=st["critic"])
        _bind_grads(policy, st, pdev)
        return scalars

    from . import _native as N
    st = _state(policy, dev, n, rows)
    with torch.no_grad():
        if normalize_advantage and n > 1:
            # the normalised minibatch advantages go back to their rows of a flat column the policy owns (a duplicate index writes the
            # same value twice), so the C call reads every column through the same indices
            if indices is None:
                st["adv"][:n] = adv
            else:
                st["adv"].index_copy_(0, indices, adv)
            adv_col = st["adv"]
        else:
            adv_col = cols["advantages"]
    r = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["log_prob"].data_ptr(), adv_col.data_ptr(), cols["returns"].data_ptr(),
                  indices.data_ptr() if indices is not None else None, rows)
    o = N.PpoOut(st["actor"].data_ptr(), st["critic"].data_ptr(), st["scalars"].data_ptr(), None, None)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = N.lib().rdv_ppo_loss_grad if route == "shipped" else N.lib().rdv_ppo_mlp_loss_grad
    N.check(call(policy._hip_handle(dev), policy._critic_handle(dev), C.byref(r), n, float(clip_range), float(ent_coef),
                 float(vf_coef), C.c_void_p(st["workspace"].data_ptr()), st["workspace"].numel(), C.byref(o), stream))
    _bind_grads(policy, st, dev)
    s = st["scalars"].clone()
    return {name: s[k] for k, name in enumerate(SCALAR_NAMES)}


# ---------------------------------------------------------------------------------------------------- the recurrent policy
def ppo_sequence_minibatches(n_envs, envs_per_batch, generator=None, device=None):
    """One epoch over the env columns of a recurrent rollout: a ``torch.randperm(n_envs)`` cut into consecutive pieces of
    ``envs_per_batch`` columns (the last may be short) — what sb3-contrib's ``RecurrentRolloutBuffer`` yields when its split falls on env
    boundaries.  Every column appears exactly once.  The tensors are marked as in range for ``n_envs``, so
    ``LstmPolicy.ppo_sequence_grad`` does not check them again."""
    n_envs, envs_per_batch = int(n_envs), int(envs_per_batch)
    if n_envs <= 0 or envs_per_batch <= 0:
        raise ValueError(f"ppo_sequence_minibatches: n_envs = {n_envs} and envs_per_batch = {envs_per_batch} must be positive")
    if device is None:
        device = generator.device if generator is not None else "cpu"
    perm = torch.randperm(n_envs, generator=generator, device=device)
    parts = list(torch.split(perm, envs_per_batch))
    for p in parts:
        p._rdv_ppo_envs = n_envs
    return parts


def _sequence_params(policy):
    """The parameters of an ``LstmPolicy`` in the order of rdv_lstm_ppo_grad_floats: per net the LSTM's w_ih, w_hh, b_ih, b_hh, then the
    trunk's layers, ``log_std`` last for the actor."""
    from .policy_lstm import _LSTM_KEYS
    actor, critic = _params(policy)
    return ([getattr(policy.lstm_actor, k) for k in _LSTM_KEYS] + actor, [getattr(policy.lstm_critic, k) for k in _LSTM_KEYS] + critic)


def _lstm_specs(policy):
    from . import _native as N
    from .policy import ACTIVATIONS
    act = ACTIVATIONS[policy.activation][0]
    return (N.LstmSpec.make(policy.lstm_hidden_size, policy.pi_arch, act), N.LstmSpec.make(policy.lstm_hidden_size, policy.vf_arch, act))


def sequence_latents(lstm, obs, start, h0, c0):
    """``h_t`` [T, B, H] of one ``torch.nn.LSTM`` layer stepped over ``obs`` [T, B, 17] from the constant ``(h0, c0)`` [B, H], the state
    multiplied by ``1 - start[t]`` ([T, B], row 0 zeros: state0 is given as step 0 sees it) in front of step t."""
    h, c, out = h0, c0, []
    for t in range(obs.shape[0]):
        keep = (1.0 - start[t])[:, None]
        _, (h1, c1) = lstm(obs[t][None], ((h * keep)[None], (c * keep)[None]))
        h, c = h1[0], c1[0]
        out.append(h)
    return torch.stack(out)


def _sequence_columns(who, buf, H, state0=None, critic_state0=None):
    """The [T, N] columns of a recurrent rollout and its two state0 pairs, checked: (cols, [(h, c) actor, (h, c) critic], T, N, device)."""
    obs = buf.get("obs")
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[2] != 17:
        raise ValueError(f"{who}: buf['obs']: expected a [T,N,17] tensor, got {tuple(getattr(obs, 'shape', ()))}")
    T, N, dev = int(obs.shape[0]), int(obs.shape[1]), obs.device
    cols = {}
    for name, shape, dtype in (("obs", (T, N, 17), torch.float32), ("actions", (T, N, 6), torch.float32), ("log_prob", (T, N), torch.float32),
                               ("advantages", (T, N), torch.float32), ("returns", (T, N), torch.float32), ("done", (T, N), torch.uint8)):
        t = buf.get(name)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{who}: buf[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev} "
                             "(what RendezvousBatch.collect returns)")
        cols[name] = t
    states = []
    for given, key, kw in ((state0, "lstm_state0", "state0"), (critic_state0, "lstm_critic_state0", "critic_state0")):
        pair = given if given is not None else buf.get(key)
        if pair is None:
            raise ValueError(f"{who}: buf holds no {key!r} (RendezvousBatch.collect records it) and {kw}= is not given")
        pair = tuple(pair)
        if len(pair) != 2 or any(not isinstance(x, torch.Tensor) or tuple(x.shape) != (N, H) for x in pair):
            raise ValueError(f"{who}: {kw} must be a pair (h, c) of [{N}, {H}] tensors")
        states.append(tuple(x.to(dev, torch.float32).contiguous() for x in pair))
    return cols, states, T, N, dev


def _sequence_state(policy, dev, T, B, N):
    st = policy.__dict__.setdefault("_ppo_seq", {}).get(dev)
    actor, critic = _sequence_params(policy)
    if st is None:
        st = dict(actor=torch.zeros(sum(p.numel() for p in actor), dtype=torch.float32, device=dev),
                  critic=torch.zeros(sum(p.numel() for p in critic), dtype=torch.float32, device=dev),
                  scalars=torch.zeros(8, dtype=torch.float32, device=dev), workspace=None, adv=None, need=0)
        policy._ppo_seq[dev] = st
    if T is not None:
        from . import _native as Nat
        a, c = _lstm_specs(policy)
        need = int(Nat.lib().rdv_lstm_ppo_workspace_bytes(C.byref(a), C.byref(c), T, B))
        if need < 0:
            raise ValueError("ppo_sequence_grad: " + Nat.lib().rdv_last_error().decode("utf-8", "replace"))
        if st["workspace"] is None or st["need"] < need:
            st["workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
            st["need"] = need
        if st["adv"] is None or st["adv"].numel() < T * N:
            st["adv"] = torch.zeros(T * N, dtype=torch.float32, device=dev)
    return st


def ppo_sequence_grad(policy, buf, envs=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True, state0=None,
                      critic_state0=None):
    """See ``LstmPolicy.ppo_sequence_grad``."""
    from .policy_lstm import LstmPolicy
    if not isinstance(policy, LstmPolicy):
        raise TypeError(f"ppo_sequence_grad: a {type(policy).__name__} is not offered: it serves one LstmPolicy (MlpPolicy has ppo_grad; "
                        "an LstmPolicySet has ppo_sequence_grads for all its members at once)")
    _check_coefficients("ppo_sequence_grad", clip_range, ent_coef, vf_coef)
    cols, states, T, N, dev = _sequence_columns("ppo_sequence_grad", buf, policy.lstm_hidden_size, state0, critic_state0)
    if envs is None:
        B = N
    else:
        if not isinstance(envs, torch.Tensor) or envs.dtype != torch.int64 or envs.dim() != 1 or envs.device != dev or envs.numel() == 0:
            raise ValueError(f"ppo_sequence_grad: envs must be a non-empty 1-d int64 tensor on {dev}")
        envs = envs.contiguous()
        B = int(envs.numel())
        if check and getattr(envs, "_rdv_ppo_envs", None) != N:
            lo, hi = (int(x) for x in torch.aminmax(envs))
            if lo < 0 or hi >= N:
                raise IndexError(f"ppo_sequence_grad: envs span [{lo}, {hi}], the rollout has columns 0..{N - 1}")
    take = (lambda t: t) if envs is None else (lambda t: t[:, envs])
    adv = take(cols["advantages"])
    if normalize_advantage and T * B > 1:
        adv = normalize_advantages(adv)
    hip = policy.backend != "torch" and dev.type == "cuda"
    actor, critic = _sequence_params(policy)

    if not hip:
        pdev = policy.log_std.device
        st = _sequence_state(policy, pdev, None, None, None)
        params = actor + critic
        flags = [p.requires_grad for p in params]
        try:
            for p in params:
                p.requires_grad_(True)
            with torch.enable_grad():
                o = take(cols["obs"]).to(pdev)
                start = torch.cat([torch.zeros_like(cols["done"][:1]), cols["done"][:-1]], dim=0)
                start = take(start).to(pdev, torch.float32)
                pick = (lambda x: x) if envs is None else (lambda x: x[envs])
                lat_a = sequence_latents(policy.lstm_actor, o, start, pick(states[0][0]).to(pdev), pick(states[0][1]).to(pdev))
                lat_c = sequence_latents(policy.lstm_critic, o, start, pick(states[1][0]).to(pdev), pick(states[1][1]).to(pdev))
                mean = policy._trunk_torch("l", lat_a).reshape(T * B, 6)
                values = policy._trunk_torch("v", lat_c).reshape(T * B)
                flat = lambda t: take(t).to(pdev).reshape((T * B,) + tuple(t.shape[2:]))
                loss, scalars, log_prob = ppo_loss_terms(mean, policy.log_std, values, flat(cols["actions"]), flat(cols["log_prob"]),
                                                         adv.to(pdev).reshape(T * B), flat(cols["returns"]), float(clip_range), float(ent_coef), float(vf_coef))
                grads = torch.autograd.grad(loss, params)
        finally:
            for p, f in zip(params, flags):
                p.requires_grad_(f)
        with torch.no_grad():
            torch.cat([g.reshape(-1) for g in grads[:len(actor)]], out=st["actor"])
            torch.cat([g.reshape(-1) for g in grads[len(actor):]], out=st["critic"])
        _bind_grads(policy, st, pdev, (actor, critic))
        policy.__dict__.pop("_ppo_seq_last", None)       # the gradients are autograd's: the adam_step behind this call is the PyTorch one
        scalars["log_prob"] = log_prob.detach().reshape(T, B)
        scalars["values"] = values.detach().reshape(T, B)
        return scalars

    from . import _native as Nat
    st = _sequence_state(policy, dev, T, B, N)
    with torch.no_grad():
        if normalize_advantage and T * B > 1:
            # the normalised advantages go back to their columns of a [T, N] array the policy owns (a duplicate column writes the same
            # values twice): the C call reads every column through the same list
            adv_col = st["adv"][:T * N].view(T, N)
            if envs is None:
                adv_col.copy_(adv)
            else:
                adv_col.index_copy_(1, envs, adv)
        else:
            adv_col = cols["advantages"]
    log_prob = torch.empty((T, B), dtype=torch.float32, device=dev)
    values = torch.empty((T, B), dtype=torch.float32, device=dev)
    r = Nat.LstmPpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["log_prob"].data_ptr(), adv_col.data_ptr(), cols["returns"].data_ptr(),
                        cols["done"].data_ptr(), states[0][0].data_ptr(), states[0][1].data_ptr(), states[1][0].data_ptr(), states[1][1].data_ptr(),
                        envs.data_ptr() if envs is not None else None, N, T, B)
    o = Nat.LstmPpoOut(st["actor"].data_ptr(), st["critic"].data_ptr(), st["scalars"].data_ptr(), log_prob.data_ptr(), values.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Nat.check(Nat.lib().rdv_lstm_ppo_loss_grad(policy._handle("l", dev), policy._handle("v", dev), C.byref(r), float(clip_range), float(ent_coef),
                                               float(vf_coef), C.c_void_p(st["workspace"].data_ptr()), st["workspace"].numel(), C.byref(o), stream))
    _bind_grads(policy, st, dev, (actor, critic))
    policy.__dict__["_ppo_seq_last"] = dev
    s = st["scalars"].clone()
    res = {name: s[k] for k, name in enumerate(SCALAR_NAMES)}
    res["log_prob"], res["values"] = log_prob, values
    return res


# ---------------------------------------------------------------------------------------------------- the recurrent set
def ppo_sequence_set_minibatches(lset, envs_per_batch, generator=None, device=None):
    """One epoch for all members of an ``LstmPolicySet`` over the env columns of a recurrent rollout: member g gets a
    ``torch.randperm(size_g)`` of its own columns, drawn in member order from the one generator, shifted to the GLOBAL columns
    ``start_g + ..`` and cut into pieces of ``envs_per_batch`` as ``ppo_sequence_minibatches`` cuts (the last may be short).  Returns a
    list of steps; step k is a list of P int64 tensors, ``None`` for a member whose pieces have run out (a smaller member).  Every column
    of every member appears exactly once.  The tensors are marked as inside their member's columns of this set, so
    ``LstmPolicySet.ppo_sequence_grads`` does not check them again."""
    envs_per_batch = int(envs_per_batch)
    if envs_per_batch <= 0:
        raise ValueError(f"ppo_sequence_set_minibatches: envs_per_batch = {envs_per_batch} must be positive")
    if device is None:
        device = generator.device if generator is not None else "cpu"
    N = int(lset.num_rows)
    per = []
    for sl in lset.group_slices:
        perm = torch.randperm(sl.stop - sl.start, generator=generator, device=device) + sl.start
        pieces = list(torch.split(perm, envs_per_batch))
        for p in pieces:
            p._rdv_ppo_seq_set = (N, sl.start, sl.stop)
        per.append(pieces)
    return [[pieces[k] if k < len(pieces) else None for pieces in per] for k in range(max(len(pieces) for pieces in per))]


def _sequence_set_state(lset, dev, P, T, N, total, counts):
    """The buffers an LstmPolicySet owns for ppo_sequence_grads on device ``dev``: the gradients [P, Ga] and [P, Gc] (row g: member g's
    flat buffers, of which its parameters' ``.grad`` are views), the scalars [P, 8], the concatenated columns, the [T, N] advantage array
    and the workspace, the last three grown when a call needs more."""
    from . import _native as Nat
    a, c = _lstm_specs(lset.policies[0])
    st = lset.__dict__.setdefault("_ppo_seq", {}).get(dev)
    if st is None:
        Ga, Gc = int(Nat.lib().rdv_lstm_ppo_grad_floats(C.byref(a), 1)), int(Nat.lib().rdv_lstm_ppo_grad_floats(C.byref(c), 0))
        st = dict(actor=torch.zeros((P, Ga), dtype=torch.float32, device=dev), critic=torch.zeros((P, Gc), dtype=torch.float32, device=dev),
                  scalars=torch.zeros((P, Nat.PPO_SCALARS), dtype=torch.float32, device=dev), envs=None, adv=None, workspace=None)
        lset._ppo_seq[dev] = st
    if st["envs"] is None or st["envs"].numel() < total:
        st["envs"] = torch.zeros(total, dtype=torch.int64, device=dev)
    if st["adv"] is None or st["adv"].numel() < T * N:
        st["adv"] = torch.zeros(T * N, dtype=torch.float32, device=dev)
    need = int(Nat.lib().rdv_lstm_ppo_set_workspace_bytes(C.byref(a), C.byref(c), T, P, counts))
    if need < 0:
        raise ValueError(f"ppo_sequence_grads: a set of {P} members is not served by one call (rdv_lstm_ppo_set_workspace_bytes)")
    if st["workspace"] is None or st["workspace"].numel() < need:
        st["workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
    return st


def ppo_sequence_set_grads(lset, buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
    """See ``LstmPolicySet.ppo_sequence_grads``."""
    from .policy_lstm import LstmPolicySet
    if not isinstance(lset, LstmPolicySet):
        raise TypeError(f"ppo_sequence_grads: a {type(lset).__name__} is not offered: it serves an LstmPolicySet (one LstmPolicy has "
                        "ppo_sequence_grad, a PolicySet ppo_grads)")
    P = len(lset)
    if not isinstance(pieces, (list, tuple)) or len(pieces) != P:
        raise ValueError(f"ppo_sequence_grads: pieces must be a list of {P} tensors (or None), one per member")
    _check_coefficients("ppo_sequence_grads", clip_range, ent_coef, vf_coef)
    cols, states, T, N, dev = _sequence_columns("ppo_sequence_grads", buf, lset.lstm_hidden_size)
    if N != lset.num_rows:
        raise ValueError(f"ppo_sequence_grads: buf['obs'] is {tuple(buf['obs'].shape)}, expected [T, {lset.num_rows}, 17]: N must be the set's rows")
    live = [g for g in range(P) if pieces[g] is not None]
    if not live:
        raise ValueError("ppo_sequence_grads: every member's piece is None")
    pieces = list(pieces)
    for g in live:
        e, sl = pieces[g], lset.group_slices[g]
        if not isinstance(e, torch.Tensor) or e.dtype != torch.int64 or e.dim() != 1 or e.device != dev or e.numel() == 0:
            raise ValueError(f"ppo_sequence_grads: pieces[{g}] must be a non-empty 1-d int64 tensor on {dev} (or None)")
        if check and getattr(e, "_rdv_ppo_seq_set", None) != (N, sl.start, sl.stop):
            lo, hi = (int(x) for x in torch.aminmax(e))
            if lo < 0 or hi >= N:
                raise IndexError(f"ppo_sequence_grads: pieces[{g}] span [{lo}, {hi}], the rollout has columns 0..{N - 1}")
            if lo < sl.start or hi >= sl.stop:
                raise IndexError(f"ppo_sequence_grads: pieces[{g}] reach env columns [{lo}, {hi}], member {g} owns {sl.start}..{sl.stop - 1}")
        pieces[g] = e.contiguous()

    if lset.backend == "torch" or dev.type != "cuda":
        out = [None] * P
        for g in live:
            member = lset[g]
            backend = member.backend
            member.backend = "torch"
            try:
                out[g] = ppo_sequence_grad(member, buf, pieces[g], clip_range, ent_coef, vf_coef, normalize_advantage, check=False)
            finally:
                member.backend = backend
        # the gradients are now in the members' own buffers, not in the set's rows: the adam_step behind this call is the PyTorch one
        lset.__dict__.pop("_ppo_seq_last", None)
        return out

    from . import _native as Nat
    counts = (C.c_int64 * P)(*[int(pieces[g].numel()) if pieces[g] is not None else 0 for g in range(P)])
    total = sum(counts)
    st = _sequence_set_state(lset, dev, P, T, N, total, counts)
    with torch.no_grad():
        torch.cat([pieces[g] for g in live], out=st["envs"][:total])
        if normalize_advantage and T * max(counts) > 1:
            # SB3's expression per member over its own [T, B_g] entries (the expression of ppo_sequence_grad: the same bits), written back
            # to the member's columns of the one [T, N] array the set owns (members own disjoint columns; a duplicate column writes the
            # same values twice); a lone entry keeps its raw advantage, as SB3 leaves it
            adv_col = st["adv"][:T * N].view(T, N)
            for g in live:
                adv = cols["advantages"][:, pieces[g]]
                adv_col.index_copy_(1, pieces[g], normalize_advantages(adv) if T * counts[g] > 1 else adv)
        else:
            adv_col = cols["advantages"]
    log_prob = torch.empty(T * total, dtype=torch.float32, device=dev)
    values = torch.empty(T * total, dtype=torch.float32, device=dev)
    r = Nat.LstmPpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["log_prob"].data_ptr(), adv_col.data_ptr(), cols["returns"].data_ptr(),
                        cols["done"].data_ptr(), states[0][0].data_ptr(), states[0][1].data_ptr(), states[1][0].data_ptr(), states[1][1].data_ptr(),
                        st["envs"].data_ptr(), N, T, total)
    o = Nat.LstmPpoSetOut(st["actor"].data_ptr(), st["critic"].data_ptr(), st["scalars"].data_ptr(), log_prob.data_ptr(), values.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Nat.check(Nat.lib().rdv_lstm_ppo_set_loss_grad(lset._handle("l", dev), lset._handle("v", dev), C.byref(r), counts, float(clip_range), float(ent_coef),
                                                   float(vf_coef), C.c_void_p(st["workspace"].data_ptr()), st["workspace"].numel(), C.byref(o), stream))
    lset._ppo_seq_last = dev
    s = st["scalars"].clone()
    out, off = [None] * P, 0
    for g in range(P):
        B = counts[g]
        if B:
            _bind_grads(lset[g], dict(actor=st["actor"][g], critic=st["critic"][g]), dev, _sequence_params(lset[g]))
            out[g] = {name: s[g, k] for k, name in enumerate(SCALAR_NAMES)}
            out[g]["log_prob"] = log_prob[T * off:T * (off + B)].view(T, B)
            out[g]["values"] = values[T * off:T * (off + B)].view(T, B)
        off += B
    return out


def _set_grad_floats(pset, route):
    """(Ga, Gc): the lengths of a member's flat actor and critic gradients."""
    from . import _native as N
    if route != "mlp":
        return N.PPO_ACTOR_GRAD, N.PPO_CRITIC_GRAD
    a, c = _specs(pset.policies[0])
    return int(N.lib().rdv_ppo_mlp_grad_floats(C.byref(a), 1)), int(N.lib().rdv_ppo_mlp_grad_floats(C.byref(c), 0))


def _set_state(pset, dev, P, total, rows, counts, route="shipped"):
    """The buffers a PolicySet owns for ppo_grads on device ``dev``: the gradients [P,Ga] and [P,Gc] (5708 and 5377 for the shipped
    architecture; row g: member g's flat buffers, of which its parameters' ``.grad`` are views), the scalars [P,8], the concatenated
    indices, the advantage column and the workspace, the last three grown when a call needs more."""
    from . import _native as N
    st = pset.__dict__.setdefault("_ppo", {}).get(dev)
    if st is None:
        Ga, Gc = _set_grad_floats(pset, route)
        st = dict(actor=torch.zeros((P, Ga), dtype=torch.float32, device=dev),
                  critic=torch.zeros((P, Gc), dtype=torch.float32, device=dev),
                  scalars=torch.zeros((P, N.PPO_SCALARS), dtype=torch.float32, device=dev), idx=None, adv=None, workspace=None)
        pset._ppo[dev] = st
    if st["idx"] is None or st["idx"].numel() < total:
        st["idx"] = torch.zeros(total, dtype=torch.int64, device=dev)
    if st["adv"] is None or st["adv"].numel() < rows:
        st["adv"] = torch.zeros(rows, dtype=torch.float32, device=dev)
    if route == "mlp":
        a, c = _specs(pset.policies[0])
        need = int(N.lib().rdv_ppo_mlp_set_workspace_bytes(C.byref(a), C.byref(c), P, counts))
    else:
        need = int(N.lib().rdv_ppo_set_workspace_bytes(P, counts))
    if need < 0:
        raise ValueError(f"ppo_grads: a set of {P} members is not served by one call (rdv_ppo_{'mlp_' if route == 'mlp' else ''}set_workspace_bytes)")
    if st["workspace"] is None or st["workspace"].numel() < need:
        st["workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
    return st


def ppo_set_grads(pset, buf, indices, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
    """See ``PolicySet.ppo_grads``."""
    from .policy import PolicySet
    if not isinstance(pset, PolicySet):
        raise TypeError(f"ppo_grads: a {type(pset).__name__} is not offered: the set form of the PPO minibatch gradients is built for "
                        "PolicySet alone (an LstmPolicySet has ppo_sequence_grads)")
    P = len(pset)
    if not isinstance(indices, (list, tuple)) or len(indices) != P:
        raise ValueError(f"ppo_grads: indices must be a list of {P} tensors (or None), one per member")
    if not pset.has_critic:
        raise ValueError("ppo_grads: a member has no critic (its weights hold no value_net trunk)")
    _check_coefficients("ppo_grads", clip_range, ent_coef, vf_coef)
    cols, rows, dev = _columns(buf)
    obs = buf["obs"]
    if obs.dim() != 3 or int(obs.shape[1]) != pset.num_rows:
        raise ValueError(f"ppo_grads: buf['obs'] is {tuple(obs.shape)}, expected [T, {pset.num_rows}, 17]: N must be the set's rows")
    n_envs = pset.num_rows
    live = [g for g in range(P) if indices[g] is not None]
    if not live:
        raise ValueError("ppo_grads: every member's indices are None")
    indices = list(indices)
    for g in live:
        idx, sl = indices[g], pset.group_slices[g]
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != dev or idx.numel() == 0:
            raise ValueError(f"ppo_grads: indices[{g}] must be a non-empty 1-d int64 tensor on {dev} (or None)")
        if check and getattr(idx, "_rdv_ppo_set", None) != (rows, n_envs, sl.start, sl.stop):
            lo, hi = (int(x) for x in torch.aminmax(idx))
            if lo < 0 or hi >= rows:
                raise IndexError(f"ppo_grads: indices[{g}] span [{lo}, {hi}], the rollout has rows 0..{rows - 1}")
            lo, hi = (int(x) for x in torch.aminmax(idx % n_envs))
            if lo < sl.start or hi >= sl.stop:
                raise IndexError(f"ppo_grads: indices[{g}] reach env columns [{lo}, {hi}], member {g} owns {sl.start}..{sl.stop - 1}")
        indices[g] = idx.contiguous()

    route = hip_set_route(pset) if dev.type == "cuda" else None
    if route is None:
        out = [None] * P
        for g in live:
            member = pset[g]
            backend = member.backend
            if pset.backend == "torch":
                member.backend = "torch"
            try:
                out[g] = ppo_grad(member, buf, indices[g], clip_range, ent_coef, vf_coef, normalize_advantage, check=False)
            finally:
                member.backend = backend
        # the gradients are now in the members' own buffers, not in the set's rows: the adam_step behind this call is the PyTorch one
        pset.__dict__.pop("_ppo_last", None)
        return out

    from . import _native as N
    counts = (C.c_int64 * P)(*[int(indices[g].numel()) if indices[g] is not None else 0 for g in range(P)])
    total = sum(counts)
    st = _set_state(pset, dev, P, total, rows, counts, route)
    with torch.no_grad():
        torch.cat([indices[g] for g in live], out=st["idx"][:total])
        if normalize_advantage and max(counts) > 1:
            # SB3's expression per member on its own 1-d minibatch (the expression of ppo_grad: the same bits), written back to the
            # member's rows of the one advantage column the set owns; a lone sample keeps its raw advantage, as SB3 leaves it
            for g in live:
                adv = cols["advantages"][indices[g]]
                st["adv"].index_copy_(0, indices[g], normalize_advantages(adv) if counts[g] > 1 else adv)
            adv_col = st["adv"]
        else:
            adv_col = cols["advantages"]
    r = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["log_prob"].data_ptr(), adv_col.data_ptr(), cols["returns"].data_ptr(),
                  st["idx"].data_ptr(), rows)
    o = N.PpoSetOut(st["actor"].data_ptr(), st["critic"].data_ptr(), st["scalars"].data_ptr(), None, None)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = N.lib().rdv_ppo_set_loss_grad if route == "shipped" else N.lib().rdv_ppo_mlp_set_loss_grad
    N.check(call(pset._hip_handle(dev), pset._critic_handle(dev), C.byref(r), counts, float(clip_range), float(ent_coef),
                 float(vf_coef), C.c_void_p(st["workspace"].data_ptr()), st["workspace"].numel(), C.byref(o), stream))
    pset._ppo_last = dev
    s = st["scalars"].clone()
    out = [None] * P
    for g in live:
        _bind_grads(pset[g], dict(actor=st["actor"][g], critic=st["critic"][g]), dev)
        out[g] = {name: s[g, k] for k, name in enumerate(SCALAR_NAMES)}
    return out


# ---------------------------------------------------------------------------------------------------- the optimiser step of a set
def _check_adam(lr, betas, eps, max_grad_norm):
    lr, eps, max_grad_norm = float(lr), float(eps), float(max_grad_norm)
    b1, b2 = (float(b) for b in betas)
    for name, v in (("lr", lr), ("eps", eps)):
        if not math.isfinite(v) or v <= 0.0:
            raise ValueError(f"adam_step: {name} = {v!r} must be finite and positive")
    for name, v in (("betas[0]", b1), ("betas[1]", b2)):
        if not 0.0 <= v < 1.0:
            raise ValueError(f"adam_step: {name} = {v!r} must be in [0, 1)")
    if not max_grad_norm > 0.0:
        raise ValueError(f"adam_step: max_grad_norm = {max_grad_norm!r} must be positive (inf: no clipping)")
    return lr, b1, b2, eps, max_grad_norm


class _MlpAdam:
    """What the optimiser step of a ``PolicySet`` takes from the set: its members, a member's (actor, critic) parameter lists in the order
    of its gradient rows, the set's gradient buffers on a device, and the device call."""
    what = "ppo_grads"

    @staticmethod
    def members(pset):
        return pset.policies

    params = staticmethod(_params)

    @staticmethod
    def grads(pset, dev):
        return pset._ppo[dev]

    @staticmethod
    def device(pset):
        dev = getattr(pset, "_ppo_last", None)
        route = hip_set_route(pset)
        if dev is None or route is None or len(pset) > 64:
            return None
        st = pset.__dict__.get("_ppo", {}).get(dev)
        return dev if st is not None and tuple(st["actor"].shape) == (len(pset), _set_grad_floats(pset, route)[0]) else None

    @staticmethod
    def call(pset, dev, ad, grads, mask, scalars):
        from . import _native as N
        call = N.lib().rdv_ppo_set_adam_step if hip_set_route(pset) == "shipped" else N.lib().rdv_ppo_mlp_set_adam_step
        N.check(call(pset._hip_handle(dev), pset._critic_handle(dev), C.byref(ad["c"]), C.c_void_p(grads["actor"].data_ptr()),
                     C.c_void_p(grads["critic"].data_ptr()), C.c_uint64(mask), *scalars, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


class _LstmAdam:
    """The same for an ``LstmPolicySet`` or, as a set of one, an ``LstmPolicy``: rows in the layout of rdv_lstm_ppo_grad_floats
    (``_sequence_params``), the buffers that ``ppo_sequence_grads`` / ``ppo_sequence_grad`` filled, rdv_lstm_ppo_set_adam_step."""
    what = "ppo_sequence_grads"

    @staticmethod
    def members(pset):
        return pset.policies if hasattr(pset, "policies") else [pset]

    params = staticmethod(_sequence_params)

    @staticmethod
    def grads(pset, dev):
        st = pset._ppo_seq[dev]
        # (a stand-alone policy keeps flat buffers: row 0 of a set of one)
        return st if st["actor"].dim() == 2 else dict(actor=st["actor"].view(1, -1), critic=st["critic"].view(1, -1))

    @staticmethod
    def device(pset):
        dev = getattr(pset, "_ppo_seq_last", None)
        if dev is None or pset.backend == "torch" or len(_LstmAdam.members(pset)) > 64:
            return None
        return dev if pset.__dict__.get("_ppo_seq", {}).get(dev) is not None else None

    @staticmethod
    def call(pset, dev, ad, grads, mask, scalars):
        from . import _native as N
        if ad.get("workspace") is None:
            a, c = _lstm_specs(_LstmAdam.members(pset)[0])
            need = int(N.lib().rdv_lstm_ppo_adam_workspace_bytes(C.byref(a), C.byref(c), len(_LstmAdam.members(pset))))
            if need < 0:
                raise ValueError("adam_step: " + N.lib().rdv_last_error().decode("utf-8", "replace"))
            ad["workspace"] = torch.empty(need, dtype=torch.uint8, device=dev)
        N.check(N.lib().rdv_lstm_ppo_set_adam_step(pset._handle("l", dev), pset._handle("v", dev), C.byref(ad["c"]), C.c_void_p(grads["actor"].data_ptr()),
                                                   C.c_void_p(grads["critic"].data_ptr()), C.c_uint64(mask), *scalars,
                                                   C.c_void_p(ad["workspace"].data_ptr()), ad["workspace"].numel(),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def _adam_kind(pset):
    from .policy import PolicySet
    return _MlpAdam if isinstance(pset, PolicySet) else _LstmAdam


def _adam_device(pset):
    """The device whose gradient buffers the last ``ppo_grads`` of this set filled through rdv_ppo_set_loss_grad or
    rdv_ppo_mlp_set_loss_grad, if the device step serves the set (``hip_set_route``, at most 64 members); None: the PyTorch fallback.
    A recurrent set or policy: the device whose buffers the last ``ppo_sequence_grads`` / ``ppo_sequence_grad`` filled through the C call."""
    return _adam_kind(pset).device(pset)


def _adam_views(pset, ad):
    """The member modules' parameters <- views of row g of the master weights ``ad`` holds (filled from the modules first), so
    ``state_dict()``, checkpoints and ``update_weights()`` see the stepped weights with no copy; ``.grad`` follows to the same device."""
    kind = _adam_kind(pset)
    dev = ad["actor_param"].device
    grads = kind.grads(pset, dev)
    with torch.no_grad():
        for g, member in enumerate(kind.members(pset)):
            parts = kind.params(member)
            for flat, params in zip((ad["actor_param"][g], ad["critic_param"][g]), parts):
                flat.copy_(torch.cat([p.detach().reshape(-1).to(dev, torch.float32) for p in params]))
                at = 0
                for p in params:
                    if p.device != dev:
                        p.grad = None
                    p.data = flat[at:at + p.numel()].view(p.shape)
                    at += p.numel()
            _bind_grads(member, dict(actor=grads["actor"][g], critic=grads["critic"][g]), dev, parts)
    ad["views"] = _adam_pointers(pset)


def _adam_pointers(pset):
    """The addresses of every parameter of every member (13 x P for the shipped architecture): what ``_adam_state`` compares to see
    whether each of them still is the view of its master row that ``_adam_views`` made."""
    kind = _adam_kind(pset)
    return [p.data_ptr() for m in kind.members(pset) for part in kind.params(m) for p in part]


def _adam_state(pset, dev):
    """The RdvAdamState buffers of a set on ``dev``, allocated on first use: master weights and moments [P,Ga] / [P,Gc] (the shapes of
    the set's gradient buffers: 5708 / 5377 for the shipped architecture), steps [P], coef [P,8]."""
    from . import _native as N
    kind = _adam_kind(pset)
    table = pset.__dict__.setdefault("_adam", {})
    ad = table.get(dev)
    if ad is None:
        grads = kind.grads(pset, dev)
        P = len(kind.members(pset))
        Ga, Gc = int(grads["actor"].shape[1]), int(grads["critic"].shape[1])
        z = lambda n: torch.zeros((P, n), dtype=torch.float32, device=dev)
        ad = dict(actor_param=z(Ga), critic_param=z(Gc), actor_m=z(Ga), actor_v=z(Ga),
                  critic_m=z(Gc), critic_v=z(Gc), step=torch.zeros(P, dtype=torch.int64, device=dev),
                  coef=z(N.ADAM_COEF), views=None)
        ad["c"] = N.AdamState(*[ad[name].data_ptr() for name, _ in N.AdamState._fields_])
        table[dev] = ad
    # (a member moved with .to(), or with new storage or a new Parameter object for ANY of its parameters, no longer aliases its row:
    # the modules are the source of truth again)
    if ad["views"] != _adam_pointers(pset):
        _adam_views(pset, ad)
    return ad


def _adam_result(coef):
    c = coef.clone()
    return dict(total_norm=c[:, 0], clip_coef=c[:, 1], skipped=c[:, 4])


def set_adam_step(pset, stepped=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
    """See ``PolicySet.adam_step``."""
    from .policy import PolicySet
    if not isinstance(pset, PolicySet):
        raise TypeError(f"adam_step: a {type(pset).__name__} is not offered: the device optimiser step is built for PolicySet alone")
    return _adam_step(pset, stepped, lr, betas, eps, max_grad_norm)


def lstm_adam_step(pset, stepped=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
    """See ``LstmPolicySet.sequence_adam_step`` and ``LstmPolicy.adam_step``."""
    from .policy_lstm import LstmPolicy, LstmPolicySet
    if not isinstance(pset, (LstmPolicy, LstmPolicySet)):
        raise TypeError(f"adam_step: a {type(pset).__name__} is not offered: the recurrent optimiser step serves LstmPolicySet and LstmPolicy")
    return _adam_step(pset, stepped, lr, betas, eps, max_grad_norm)


def _adam_step(pset, stepped, lr, betas, eps, max_grad_norm):
    kind = _adam_kind(pset)
    members = kind.members(pset)
    P = len(members)
    if stepped is not None and (not isinstance(stepped, (list, tuple)) or len(stepped) != P):
        raise ValueError(f"adam_step: stepped must be the list of {P} entries that {kind.what} returned (or None: all members step)")
    lr, b1, b2, eps, max_grad_norm = _check_adam(lr, betas, eps, max_grad_norm)
    live = [g for g in range(P) if stepped is None or stepped[g] is not None]
    if not live:
        raise ValueError("adam_step: every member sits out")
    dev = kind.device(pset)
    if dev is not None:
        ad = _adam_state(pset, dev)
        mask = 0
        for g in live:
            mask |= 1 << g
        kind.call(pset, dev, ad, kind.grads(pset, dev), mask, (lr, b1, b2, eps, max_grad_norm))
        return _adam_result(ad["coef"])

    # ---- the fallback: per-member clip_grad_norm_ and ONE torch.optim.Adam over all members' parameters; the moments are PyTorch's
    fb = pset.__dict__.get("_adam_torch")
    params = [list(m.parameters()) for m in members]                 # the order of INTEGRATION.md's clip_grad_norm_(member.parameters(), ...)
    pdev = params[0][0].device
    if fb is None or fb["ids"] != [id(p) for ps in params for p in ps]:
        fb = dict(opt=torch.optim.Adam([p for ps in params for p in ps], lr=lr, betas=(b1, b2), eps=eps), ids=[id(p) for ps in params for p in ps],
                  coef=torch.zeros((P, 8), dtype=torch.float32, device=pdev))
        pset._adam_torch = fb
    for group in fb["opt"].param_groups:
        group["lr"], group["betas"], group["eps"] = lr, (b1, b2), eps
    for g in live:
        if any(p.grad is None for p in params[g]):
            raise ValueError(f"adam_step: member {g} has no gradients ({kind.what} fills them)")
    parked = {}
    for g in range(P):
        total = torch.nn.utils.clip_grad_norm_(params[g], max_grad_norm).to(torch.float32) if g in live else None
        finite = total is not None and bool(torch.isfinite(total))
        if total is not None:
            row = fb["coef"][g]
            row.zero_()
            row[0] = total
            if finite:
                row[1] = torch.clamp(max_grad_norm / (total + 1e-6), max=1.0)
            else:
                row[4] = 1.0
        if not finite:                                  # sits out or is skipped: the one optimiser passes over parameters without .grad
            for p in params[g]:
                parked[p] = p.grad
                p.grad = None
    try:
        fb["opt"].step()
    finally:
        for p, grad in parked.items():
            p.grad = grad
    dst = getattr(pset, "_ppo_last" if kind is _MlpAdam else "_ppo_seq_last", None)
    return _adam_result(fb["coef"] if dst is None or pset.backend == "torch" else fb["coef"].to(dst))


def set_reset_optimizer(pset, member=None):
    """See ``PolicySet.reset_optimizer``."""
    kind = _adam_kind(pset)
    members = kind.members(pset)
    P = len(members)
    todo = list(range(P)) if member is None else [int(member)]
    if not all(0 <= g < P for g in todo):
        raise IndexError(f"reset_optimizer: member {member} of {P}")
    with torch.no_grad():
        for ad in pset.__dict__.get("_adam", {}).values():
            for name in ("actor_m", "actor_v", "critic_m", "critic_v", "step"):
                ad[name][todo] = 0
    fb = pset.__dict__.get("_adam_torch")
    if fb is not None:
        for g in todo:
            for part in kind.params(members[g]):
                for p in part:
                    fb["opt"].state.pop(p, None)

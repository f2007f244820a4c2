"""
Reference of the PPO minibatch loss and its gradients for ANY network of tests/policy_mlp_reference.py (include/rdv.h, "PPO minibatch
gradients for every MLP architecture"; csrc/rdv_ppo_mlp.h): tests/ppo_reference.py generalised from the 17-64-64 tanh pair to 1..4 hidden
layers of 16 / 32 / 64 with tanh, ReLU or sigmoid, actor and critic each of an architecture of its own.  Twice and independently:

  * ``analytic64``: the loss of SB3's ``PPO.train()`` body and its ANALYTIC gradients in NumPy float64.  Architecture and activation are
    read from the net dicts.  The ReLU is the kernel's: capped to [0, 63], derivative 1 where 0 < h < 63 and 0 elsewhere (PyTorch's 0 at
    the kink; 0 where the cap acted).  On a 64-64 tanh pair it is ``ppo_reference.analytic64`` exactly.
  * ``autograd``: the same loss over torch modules, differentiated by autograd in double (the reference of the analytic form) or in float
    (the yardstick e32 of the GPU test).

``make_case(arch_pi, arch_vf, act)`` builds the inputs of tests/test_gpu_ppo_mlp_grad.py by the recipe of ``ppo_reference.make_case`` with
``policy_mlp_reference.dense`` networks, and asserts the conditions under which the comparison measures the kernel (the clip guard, and for
ReLU a guard around 0 of every hidden pre-activation).  Runs on the CPU; pinned by tests/test_ppo_mlp_grad.py.
"""
import functools

import numpy as np

import policy_mlp_reference as M
import policy_reference as R
import ppo_reference as P
from ppo_reference import COLUMNS, EPS, GUARD, LOG_2PI, ROWS, SCALARS, class_shares, clip_gradient_factor, index_vector, rel_err, take, with_columns, with_nan

PRE_GUARD = 1e-4                                     # ReLU: no fp64 hidden pre-activation of a case within this of 0
WRONG = ("other_activation", "relu_one_at_zero", "padded_leak", "no_backward_clamp")
SHAPES = (1, 33, 257, 549)                           # a lone lane, a wave's edge, a workgroup's edge, three workgroups with a 37-row last wave
SMALL_GROUP_SHAPES = (127, 128, 129)                 # the edge of a 128-row workgroup (blocks that leave the LDS room for four waves only)
# the smallest set that reaches every (tiles of h_l, k-steps of delta_l) shape of the backward loop, every head k-step count and depths
# 1..4; then actor != critic, [64, 64] ReLU, and [16, 16] sigmoid for the one forward shape (one tile, one k-step) the others leave out
ARCHS = ([16], [64], [32, 16], [16, 64], [64, 32, 16], [32, 16, 64, 32], [64, 64, 64, 64])
ALL_ACTS = ([32, 16], [16, 64], [64, 64, 64, 64])    # these with each of the three activations
CASES = ([(a, a, "tanh") for a in ARCHS] + [(a, a, act) for a in ALL_ACTS for act in ("relu", "sigmoid")]
         + [([32, 32], [64, 16], "relu"), ([64, 64], [64, 64], "relu"), ([16, 16], [16, 16], "sigmoid")])


def case_id(case):
    pi, vf, act = case
    return f"{M.arch_id(pi)}-{M.arch_id(vf)}-{act}" if pi != vf else f"{M.arch_id(pi)}-{act}"


def names(actor, critic):
    """The gradient tensors in the order of actor_grad, critic_grad: actor.w1, actor.b1, ..., actor.log_std, critic.w1, ..."""
    out = []
    for who, net in (("actor", actor), ("critic", critic)):
        for l in range(len(net["w"])):
            out += [f"{who}.w{l + 1}", f"{who}.b{l + 1}"]
        if who == "actor":
            out.append("actor.log_std")
    return tuple(out)


def shapes(net, actor):
    """The shapes of a net's gradient tensors in the order of its flat gradient."""
    out = []
    for w in net["w"]:
        out += [tuple(w.shape), (w.shape[0],)]
    return out + ([(6,)] if actor else [])


def actor_names(actor, critic):
    n = names(actor, critic)
    k = 2 * len(actor["w"]) + 1
    return n[:k], n[k:]


# ------------------------------------------------------------------------------------------------------------ forward and backward
def _forward64(net, x):
    """(hidden pre-activations z_1..z_L, hidden activations h_1..h_L, output) in float64 for clamped rows x"""
    f = lambda a: a.astype(np.float64)
    zs, hs, h = [], [], x
    for w, b in zip(net["w"][:-1], net["b"][:-1]):
        z = h @ f(w).T + f(b)
        h = M.activation(net["act"], z)
        zs.append(z); hs.append(h)
    return zs, hs, h @ f(net["w"][-1]).T + f(net["b"][-1])


def act_derivative(act, h, wrong=None):
    """The derivative of the activation from the activation h itself (the rule of include/rdv.h)."""
    if wrong == "other_activation":
        act = {"tanh": "sigmoid", "sigmoid": "tanh", "relu": "tanh"}[act]
    if act == "tanh":
        return 1.0 - h ** 2
    if act == "sigmoid":
        return h * (1.0 - h)
    if wrong == "relu_one_at_zero":
        return ((h >= 0.0) & (h < M.RELU_CLAMP)).astype(np.float64)
    if wrong == "relu_open_cap":                      # (beside WRONG: the derivative of an uncapped ReLU, for ``relu_clamp_case``)
        return (h > 0.0).astype(np.float64)
    return ((h > 0.0) & (h < M.RELU_CLAMP)).astype(np.float64)


def _backward64(net, x, hs, d_out, wrong=None, x_w1=None):
    """[dW_1, db_1, ..., dW_head, db_head] from the head's error d_out [n, out]; x_w1: the rows dW_1 is contracted with, when not x"""
    f = lambda a: a.astype(np.float64)
    inputs = [x if x_w1 is None else x_w1] + hs
    grads, d = [], d_out
    for l in range(len(net["w"]) - 1, -1, -1):
        dw = d.T @ inputs[l]
        if wrong == "padded_leak" and l > 0 and inputs[l].shape[1] == 16:      # a 16-wide layer read as 32 wide: 0.5 in its padded rows
            dw = dw + d.T @ np.full_like(inputs[l], 0.5)
        grads = [dw, d.sum(0)] + grads
        if l > 0:
            d = (d @ f(net["w"][l])) * act_derivative(net["act"], hs[l - 1], wrong)
    return grads


def analytic64(actor, critic, obs, actions, old_log_prob, adv, ret, eps=EPS, ent_coef=0.0, vf_coef=0.5, wrong=None):
    """dict(grads=[arrays in ``names`` order], scalars={...}, log_prob, values, ratio, mean, pre=(actor z's, critic z's), hidden=(...)) in
    float64 from float32 inputs.  wrong: one of WRONG — a wrong restatement the accuracy rule must tell from the right one."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x, a, old, A, ret = f(R.clamp_obs(np.asarray(obs, np.float32))), f(actions), f(old_log_prob), f(adv), f(ret)
    x_w1 = f(obs) if wrong == "no_backward_clamp" else None
    n = x.shape[0]
    ls = f(actor["log_std"])
    var = np.exp(2.0 * ls)
    za, ha, mu = _forward64(actor, x)
    d = a - mu
    lp = (-(d ** 2) / (2.0 * var) - ls - 0.5 * LOG_2PI).sum(1)
    ratio = np.exp(lp - old)
    s1, s2 = A * ratio, A * np.clip(ratio, 1.0 - eps, 1.0 + eps)
    g_lp = -(A * clip_gradient_factor(ratio, A, eps)) * ratio / n
    ga = _backward64(actor, x, ha, g_lp[:, None] * d / var, wrong, x_w1)
    ga.append((g_lp[:, None] * (d ** 2 / var - 1.0)).sum(0) - ent_coef)
    zc, hc, v = _forward64(critic, x)
    v = v[:, 0]
    gc = _backward64(critic, x, hc, (2.0 * vf_coef * (v - ret) / n)[:, None], wrong, x_w1)
    policy_loss, value_loss = -np.minimum(s1, s2).mean(), ((ret - v) ** 2).mean()
    entropy_loss = -float((0.5 + 0.5 * LOG_2PI + ls).sum())
    scalars = dict(loss=policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss=policy_loss, value_loss=value_loss,
                   entropy_loss=entropy_loss, approx_kl=((ratio - 1.0) - (lp - old)).mean(), clip_fraction=(np.abs(ratio - 1.0) > eps).mean())
    return dict(grads=ga + gc, scalars=scalars, log_prob=lp, values=v, ratio=ratio, mean=mu, pre=(za, zc), hidden=(ha, hc))


def autograd(actor, critic, obs, actions, old_log_prob, adv, ret, eps=EPS, ent_coef=0.0, vf_coef=0.5, dtype="float64"):
    """The same loss over torch.nn modules in ``dtype``, differentiated by autograd: (gradients as float64 arrays, scalars as floats).
    The capped ReLU is relu followed by ``where(h < 63, h, 63)``: gradient 0 at the kink (PyTorch's relu) and 0 where the cap acted."""
    import torch
    dt = getattr(torch, dtype)
    t = lambda a: torch.as_tensor(np.array(a, np.float32)).to(dt)

    def modules(net):
        lins = []
        for w, b in zip(net["w"], net["b"]):
            lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dt)
            with torch.no_grad():
                lin.weight.copy_(t(w)); lin.bias.copy_(t(b))
            lins.append(lin)
        return lins

    def fn(name, z):
        if name == "tanh":
            return torch.tanh(z)
        if name == "sigmoid":
            return torch.sigmoid(z)
        h = torch.relu(z)
        return torch.where(h < M.RELU_CLAMP, h, torch.full_like(h, M.RELU_CLAMP))

    def run(lins, name, x):
        for lin in lins[:-1]:
            x = fn(name, lin(x))
        return lins[-1](x)

    pi, vf = modules(actor), modules(critic)
    log_std = torch.nn.Parameter(t(actor["log_std"]))
    x = t(R.clamp_obs(np.asarray(obs, np.float32)))
    mean = run(pi, actor["act"], x)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp(), validate_args=False)
    log_prob, entropy = dist.log_prob(t(actions)).sum(dim=1), dist.entropy().sum(dim=1)
    values = run(vf, critic["act"], x).flatten()
    advantages, old = t(adv), t(old_log_prob)
    ratio = torch.exp(log_prob - old)
    policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - eps, 1 + eps)).mean()
    value_loss = torch.nn.functional.mse_loss(t(ret), values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    params = [p for lin in pi for p in (lin.weight, lin.bias)] + [log_std] + [p for lin in vf for p in (lin.weight, lin.bias)]
    grads = torch.autograd.grad(loss, params)
    with torch.no_grad():
        log_ratio = log_prob - old
        approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        clip_fraction = torch.mean((torch.abs(ratio - 1) > eps).to(dt))
    scalars = dict(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, approx_kl=approx_kl, clip_fraction=clip_fraction)
    return [g.detach().to(torch.float64).numpy() for g in grads], {k: float(v.detach()) for k, v in scalars.items()}


# ------------------------------------------------------------------------------------------------------------ inputs
def nets(arch_pi, arch_vf, act, seed=5):
    """Dense random actor and critic with log_std in [-1.4, -0.4] (the recipe of ``ppo_reference.random_nets``)."""
    a = M.dense(list(arch_pi), act, seed=seed)
    a["log_std"] = np.random.default_rng([seed, 77]).uniform(-1.4, -0.4, size=6).astype(np.float32)
    return a, M.critic_of(M.dense(list(arch_vf), act, seed=seed + 1))


def _pre32_error(net, x32):
    """max |float32 - fp64| over the hidden pre-activations of a net on the clamped float32 rows x32"""
    zs64 = _forward64(net, x32.astype(np.float64))[0]
    worst, h = 0.0, x32
    for l, (w, b) in enumerate(zip(net["w"][:-1], net["b"][:-1])):
        z = h @ w.T + b
        assert z.dtype == np.float32
        worst = max(worst, float(np.abs(z.astype(np.float64) - zs64[l]).max()))
        h = M.activation(net["act"], z)
    return worst


def _near_zero(nets_, x):
    """rows of which an fp64 hidden pre-activation of one of the nets lies within PRE_GUARD of 0"""
    bad = np.zeros(x.shape[0], bool)
    for net in nets_:
        for z in _forward64(net, x)[0]:
            bad |= (np.abs(z) < PRE_GUARD).any(1)
    return bad


@functools.lru_cache(maxsize=None)
def _make_case(arch_pi, arch_vf, act, seed, rows):
    actor, critic = nets(arch_pi, arch_vf, act)
    rng = np.random.default_rng([seed, 40, M.ACTS.index(act)] + list(arch_pi) + [0] + list(arch_vf))
    obs = rng.uniform(-1.0, 1.0, size=(rows, 17)).astype(np.float32)
    redrawn = 0
    if act == "relu":                                 # a pre-activation that close to 0 flips a unit's class on a last-bit difference
        for _ in range(100):
            bad = _near_zero((actor, critic), R.clamp_obs(obs).astype(np.float64))
            if not bad.any():
                break
            redrawn += int(bad.sum())
            obs[bad] = rng.uniform(-1.0, 1.0, size=(int(bad.sum()), 17)).astype(np.float32)
        assert not bad.any()
    x = R.clamp_obs(obs).astype(np.float64)
    ls = actor["log_std"].astype(np.float64)
    mu = _forward64(actor, x)[2]
    actions = (mu + np.exp(ls) * rng.standard_normal((rows, 6))).astype(np.float32)
    lp = (-((actions.astype(np.float64) - mu) ** 2) / (2.0 * np.exp(2.0 * ls)) - ls - 0.5 * LOG_2PI).sum(1)
    u = rng.uniform(-0.6, 0.6, size=rows)
    for _ in range(100):
        old = (lp - u).astype(np.float32)
        ratio = np.exp(lp - old.astype(np.float64))
        bad = (np.abs(ratio - (1.0 - EPS)) < GUARD) | (np.abs(ratio - (1.0 + EPS)) < GUARD)
        if not bad.any():
            break
        u[bad] = rng.uniform(-0.6, 0.6, size=int(bad.sum()))
    assert not bad.any()
    case = dict(actor=actor, critic=critic, obs=obs, actions=actions, old_log_prob=old,
                advantages=rng.standard_normal(rows).astype(np.float32), returns=rng.standard_normal(rows).astype(np.float32), redrawn=redrawn)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def make_case(arch_pi, arch_vf, act, seed=3, rows=ROWS):
    """The rows of the GPU test for one pair of architectures, computed once and shared: dict(actor, critic, obs, actions, old_log_prob,
    advantages, returns, redrawn).  The recipe of ``ppo_reference.make_case``; for ReLU, rows with an fp64 hidden pre-activation of the
    actor or the critic within PRE_GUARD of 0 are redrawn (deterministically) until none is left; ``redrawn`` counts them."""
    return _make_case(tuple(arch_pi), tuple(arch_vf), act, seed, rows)


def case_conditions(case, n=549):
    """What tests/test_ppo_mlp_grad.py asserts per case, from the reference alone: dict(near_zero, pre32, shares, live, top)."""
    actor, critic = case["actor"], case["critic"]
    x32 = R.clamp_obs(case["obs"])
    ref = analytic64(actor, critic, *take(case, n), eps=EPS)
    live = [float((h > 0).mean()) for hs in ref["hidden"] for h in hs]
    top = max(float(h.max()) for hs in ref["hidden"] for h in hs)
    return dict(near_zero=int(_near_zero((actor, critic), x32.astype(np.float64)).sum()), pre32=max(_pre32_error(actor, x32), _pre32_error(critic, x32)),
                shares=class_shares(ref["ratio"], case["advantages"][:n].astype(np.float64)), live=live, top=top)


def relu_clamp_case(rows=40):
    """The ReLU cap: ``policy_mlp_reference.relu_clamp_net`` ([32, 32] ReLU; unit 0 of layer 1 reads 200 x feature 0 alone) as actor and
    critic on ``relu_clamp_rows``, whose rows ``at`` drive that unit to 62.9, 63, 64 and 1e4.  Rows at or above 63 contribute nothing through
    the unit: row 0 of dW1 and db1[0] come from the other rows alone.  The row at 63 sits on the cap's edge — 200 x float32(0.315) is
    62.9999995 in fp64 and 63 in float32, so its class is decided by a last bit — and is given no weight: advantage 0, and the fp64 value
    as its return (the GPU test puts the device's own value there, which makes the critic's error of that row exactly zero).
    Returns (case, at)."""
    actor = M.relu_clamp_net()
    actor["log_std"] = np.random.default_rng([5, 77]).uniform(-1.4, -0.4, size=6).astype(np.float32)
    critic = M.critic_of(M.relu_clamp_net(seed=33))
    obs, at = M.relu_clamp_rows(rows)
    rng = np.random.default_rng([3, 41])
    x = R.clamp_obs(obs).astype(np.float64)
    ls = actor["log_std"].astype(np.float64)
    mu = _forward64(actor, x)[2]
    actions = (mu + np.exp(ls) * rng.standard_normal((rows, 6))).astype(np.float32)
    lp = (-((actions.astype(np.float64) - mu) ** 2) / (2.0 * np.exp(2.0 * ls)) - ls - 0.5 * LOG_2PI).sum(1)
    old = (lp - rng.uniform(-0.15, 0.15, size=rows)).astype(np.float32)          # every ratio inside the clip range: every row has a gradient
    adv, ret = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    adv[at[1]] = 0.0
    ret[at[1]] = np.float32(_forward64(critic, x)[2][at[1], 0])
    case = dict(actor=actor, critic=critic, obs=np.ascontiguousarray(obs, np.float32), actions=actions, old_log_prob=old, advantages=adv, returns=ret)
    return case, at


def clamp_case(rows=ROWS):
    """The +-63 observation clamp on [32, 16] ReLU: the recipe of ``ppo_reference.clamp_nets`` (column CLAMP_COL of both first-layer
    matrices times 2^-7, every CLAMP_EVERY-th row carrying CLAMP_VALUES in that feature).  The ReLU guard is asserted, not enforced by
    redrawing (the special rows must stay)."""
    base = make_case([32, 16], [32, 16], "relu")
    actor, critic = dict(base["actor"]), dict(base["critic"])
    for net in (actor, critic):
        w = [a.copy() for a in net["w"]]
        w[0][:, P.CLAMP_COL] *= np.float32(2.0 ** -7)
        net["w"] = w
    rng = np.random.default_rng([3, 42])
    obs = np.array(base["obs"])
    at = np.arange(0, rows, P.CLAMP_EVERY)
    obs[at, P.CLAMP_COL] = np.asarray(P.CLAMP_VALUES, np.float32)[np.arange(at.size) % len(P.CLAMP_VALUES)]
    for _ in range(100):
        bad = _near_zero((actor, critic), R.clamp_obs(obs).astype(np.float64))
        if not bad.any():
            break
        cols = np.setdiff1d(np.arange(17), [P.CLAMP_COL])
        obs[np.ix_(bad, cols)] = rng.uniform(-1.0, 1.0, size=(int(bad.sum()), 16)).astype(np.float32)
    assert not bad.any()
    x = R.clamp_obs(obs).astype(np.float64)
    ls = actor["log_std"].astype(np.float64)
    mu = _forward64(actor, x)[2]
    actions = (mu + np.exp(ls) * rng.standard_normal((rows, 6))).astype(np.float32)
    lp = (-((actions.astype(np.float64) - mu) ** 2) / (2.0 * np.exp(2.0 * ls)) - ls - 0.5 * LOG_2PI).sum(1)
    u = rng.uniform(-0.6, 0.6, size=rows)
    for _ in range(100):
        old = (lp - u).astype(np.float32)
        ratio = np.exp(lp - old.astype(np.float64))
        bad = (np.abs(ratio - (1.0 - EPS)) < GUARD) | (np.abs(ratio - (1.0 + EPS)) < GUARD)
        if not bad.any():
            break
        u[bad] = rng.uniform(-0.6, 0.6, size=int(bad.sum()))
    assert not bad.any()
    return dict(actor=actor, critic=critic, obs=obs, actions=actions, old_log_prob=old, advantages=np.array(base["advantages"]), returns=np.array(base["returns"]))


# ------------------------------------------------------------------------------------------------------------ the NaN rule, budgets
def nan_rule(actor, critic):
    """``ppo_reference.NAN_RULE`` with the names generalised: column -> (gradient tensors that are NaN throughout, NaN scalars)."""
    a, c = actor_names(actor, critic)
    return {"obs": (a + c, ("loss", "policy_loss", "value_loss", "approx_kl")),
            "actions": (a, ("loss", "policy_loss", "approx_kl")),
            "old_log_prob": (a, ("loss", "policy_loss", "approx_kl")),
            "advantages": (a, ("loss", "policy_loss")),
            "returns": (c, ("loss", "value_loss"))}


def nan_pattern(actor, critic, grads, scalars):
    """(names of the gradient tensors that are NaN in every entry, names of the NaN scalars); a tensor is all-NaN or finite throughout."""
    bad_names = []
    for name, g in zip(names(actor, critic), grads):
        bad = np.isnan(np.asarray(g))
        assert bad.all() or (not bad.any() and np.isfinite(np.asarray(g)).all()), name
        if bad.all():
            bad_names.append(name)
    return tuple(bad_names), tuple(k for k in SCALARS if np.isnan(scalars[k]))


def log_prob_budget(actor, obs, actions):
    """``ppo_reference.log_prob_budget`` with the means' budget of this network (1.5 e32 + A of ``policy_mlp_reference.bounds``)."""
    x32 = R.clamp_obs(np.asarray(obs, np.float32))
    _, e32, a_entry = M.bounds(actor, x32)
    ls = actor["log_std"].astype(np.float64)
    var = np.exp(2.0 * ls)
    d = np.asarray(actions, np.float64) - _forward64(actor, x32.astype(np.float64))[2]
    t = d ** 2 / (2.0 * var)
    size = (t + np.abs(ls)).sum(1) + 3.0 * LOG_2PI
    return (np.abs(d) / var).sum(1) * (1.5 * e32 + a_entry) + 2.0 ** -24 * (8.0 * t.sum(1) + 8.0 * size)

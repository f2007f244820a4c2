"""
Reference of the PPO minibatch loss and its gradients (include/rdv.h, "PPO minibatch gradients"; csrc/rdv_ppo.h) for a 17-64-64 tanh actor
and critic, twice and independently:

  * ``analytic64``: the loss of SB3's ``PPO.train()`` body (stable_baselines3/ppo/ppo.py:203-260 — ratio, the two surrogate terms and
    their ``th.min``, ``F.mse_loss(rollout_data.returns, values_pred)``, ``-th.mean(entropy)``, approx_kl, clip_fraction; the Gaussian of
    common/distributions.py:160-199, ``DiagGaussianDistribution.log_prob`` / ``.entropy``) and its ANALYTIC gradients in NumPy float64;
  * ``autograd``: the same loss written with torch modules, differentiated by autograd, in double (the reference of the analytic form) or
    in float (the yardstick e32 of the GPU test: what PyTorch's own float32 backward costs against fp64).

Networks are the dicts of tests/policy_mlp_reference.py (``w``, ``b``, ``log_std``: float32 arrays in SB3's layout).  ``make_case`` builds
the inputs of tests/test_gpu_ppo_grad.py and asserts the conditions under which the comparison measures the kernel; beside the default
1,200-row cases it builds a 65,536-row one (``big_case``), the index vector of a million samples that repeat 4,096 rows, a third member
for the observation clamp, and the degenerate variants of the random member's case (no policy gradient in chosen rows, advantages over
ten decades, one NaN).  Runs on the CPU;
pinned by tests/test_ppo_grad.py.  stable_baselines3 is not needed.
"""
import functools
import os

import numpy as np

import policy_mlp_reference as M
import policy_reference as R

LOG_2PI = float(np.log(2.0 * np.pi))
NAMES = ("actor.w1", "actor.b1", "actor.w2", "actor.b2", "actor.w3", "actor.b3", "actor.log_std",
         "critic.w1", "critic.b1", "critic.w2", "critic.b2", "critic.w3", "critic.b3")          # the order of actor_grad, critic_grad
SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
ROWS, EPS = 1200, 0.25
SHAPES = (1, 31, 32, 33, 256, 257, 549)
GUARD = 1e-4
WRONG = ("open_clip", "wrong_h", "no_entropy")       # three wrong restatements the bound must tell from the right one
BIG_ROWS, BIG_SHAPES = 65536, (4096, 65536)          # 16 and 256 workgroups, rows in order
REPEAT_BASE, REPEAT_TIMES = 4096, 256                # 1,048,576 samples = 4,096 workgroups: the first REPEAT_BASE rows, REPEAT_TIMES times each
CLAMP_VALUES = (62.9, 63.0, 64.0, 1e4, -64.0, -1e4)  # feature 3 of every eighth row of the "clamp" member's case, cyclically
CLAMP_COL, CLAMP_EVERY = 3, 8


def _forward64(net, x):
    f = lambda a: a.astype(np.float64)
    h1 = np.tanh(x @ f(net["w"][0]).T + f(net["b"][0]))
    h2 = np.tanh(h1 @ f(net["w"][1]).T + f(net["b"][1]))
    return h1, h2, h2 @ f(net["w"][2]).T + f(net["b"][2])


def _backward64(net, x, h1, h2, d3, wrong=None, x_w1=None):
    """[dW1, db1, dW2, db2, dW3, db3] from the head's error d3 [n, out]; x_w1: the rows dW1 is contracted with, when not x"""
    f = lambda a: a.astype(np.float64)
    t2, t1 = (h1, h2) if wrong == "wrong_h" else (h2, h1)          # wrong_h: tanh' from the other layer's activations
    d2 = (d3 @ f(net["w"][2])) * (1.0 - t2 ** 2)
    d1 = (d2 @ f(net["w"][1])) * (1.0 - t1 ** 2)
    return [d1.T @ (x if x_w1 is None else x_w1), d1.sum(0), d2.T @ h1, d2.sum(0), d3.T @ h2, d3.sum(0)]


def clip_gradient_factor(ratio, adv, eps, wrong=None):
    """d min(A ratio, A clamp(ratio, 1 - eps, 1 + eps)) / d ratio, over A: PyTorch's min / clamp backward (rdv.h)."""
    inside = (ratio >= 1.0 - eps) & (ratio <= 1.0 + eps)
    unclipped_smaller = adv * ratio < adv * np.clip(ratio, 1.0 - eps, 1.0 + eps)
    if wrong == "open_clip":                                        # the rule without the interior of the inclusive limits
        return unclipped_smaller.astype(np.float64)
    return (inside | unclipped_smaller).astype(np.float64)


def analytic64(actor, critic, obs, actions, old_log_prob, adv, ret, eps=EPS, ent_coef=0.0, vf_coef=0.5, wrong=None):
    """dict(grads=[13 arrays in NAMES order], scalars={...}, log_prob, values, ratio, mean, h1, c1) in float64 from float32 inputs.
    wrong="no_backward_clamp": a fourth wrong restatement — the forward pass of the clamped rows, dW1 contracted with the rows as given."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    x, a, old, A, ret = f(R.clamp_obs(np.asarray(obs, np.float32))), f(actions), f(old_log_prob), f(adv), f(ret)
    x_w1 = f(obs) if wrong == "no_backward_clamp" else None
    n = x.shape[0]
    ls = f(actor["log_std"])
    var = np.exp(2.0 * ls)
    h1, h2, mu = _forward64(actor, x)
    d = a - mu
    lp = (-(d ** 2) / (2.0 * var) - ls - 0.5 * LOG_2PI).sum(1)
    ratio = np.exp(lp - old)
    s1, s2 = A * ratio, A * np.clip(ratio, 1.0 - eps, 1.0 + eps)
    g_lp = -(A * clip_gradient_factor(ratio, A, eps, wrong)) * ratio / n          # d loss / d log_prob_i
    ga = _backward64(actor, x, h1, h2, g_lp[:, None] * d / var, wrong, x_w1)
    ga.append((g_lp[:, None] * (d ** 2 / var - 1.0)).sum(0) - (0.0 if wrong == "no_entropy" else ent_coef))
    c1, c2, v = _forward64(critic, x)
    v = v[:, 0]
    gc = _backward64(critic, x, c1, c2, (2.0 * vf_coef * (v - ret) / n)[:, None], wrong, x_w1)
    policy_loss, value_loss = -np.minimum(s1, s2).mean(), ((ret - v) ** 2).mean()
    entropy_loss = -float((0.5 + 0.5 * LOG_2PI + ls).sum())
    scalars = dict(loss=policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss=policy_loss, value_loss=value_loss,
                   entropy_loss=entropy_loss, approx_kl=((ratio - 1.0) - (lp - old)).mean(), clip_fraction=(np.abs(ratio - 1.0) > eps).mean())
    return dict(grads=ga + gc, scalars=scalars, log_prob=lp, values=v, ratio=ratio, mean=mu, h1=h1, c1=c1)


def autograd(actor, critic, obs, actions, old_log_prob, adv, ret, eps=EPS, ent_coef=0.0, vf_coef=0.5, dtype="float64"):
    """The same loss over torch.nn modules in ``dtype``, differentiated by autograd: (13 gradients as float64 arrays, scalars as floats)."""
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

    def run(lins, x):
        return lins[2](torch.tanh(lins[1](torch.tanh(lins[0](x)))))

    pi, vf = modules(actor), modules(critic)
    log_std = torch.nn.Parameter(t(actor["log_std"]))
    x = t(R.clamp_obs(np.asarray(obs, np.float32)))
    dist = torch.distributions.Normal(run(pi, x), torch.ones_like(run(pi, x)) * log_std.exp(), validate_args=False)   # distributions.py:166-168 (a NaN row is an input here, not a mistake)
    log_prob, entropy = dist.log_prob(t(actions)).sum(dim=1), dist.entropy().sum(dim=1)            # sum_independent_dims
    values = run(vf, x).flatten()
    advantages, old = t(adv), t(old_log_prob)
    ratio = torch.exp(log_prob - old)                                                              # ppo.py:221
    policy_loss_1 = advantages * ratio
    policy_loss_2 = advantages * torch.clamp(ratio, 1 - eps, 1 + eps)
    policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()                                  # ppo.py:224-226
    value_loss = torch.nn.functional.mse_loss(t(ret), values)                                      # ppo.py:243
    entropy_loss = -torch.mean(entropy)                                                            # ppo.py:251
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss                            # ppo.py:255
    params = [p for lin in pi for p in (lin.weight, lin.bias)] + [log_std] + [p for lin in vf for p in (lin.weight, lin.bias)]
    grads = torch.autograd.grad(loss, params)
    with torch.no_grad():
        log_ratio = log_prob - old
        approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)                             # ppo.py:262-263
        clip_fraction = torch.mean((torch.abs(ratio - 1) > eps).to(dt))                            # ppo.py:231
    scalars = dict(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, approx_kl=approx_kl, clip_fraction=clip_fraction)
    return [g.detach().to(torch.float64).numpy() for g in grads], {k: float(v.detach()) for k, v in scalars.items()}


def rel_err(got, want):
    """max|got - want| / max|want| of one tensor (the quantity of the accuracy rule)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------ inputs
def golden_nets():
    """Actor and critic of tests/golden/mlp_policy.npz as policy_mlp_reference networks."""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_policy.npz"), allow_pickle=False))
    w = lambda keys: [np.asarray(g[k], np.float32) for k in keys]
    a = M.make_net(w(["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.2.weight", "action_net.weight"]),
                   w(["mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.bias", "action_net.bias"]), "tanh", g["log_std"])
    c = M.make_net(w(["mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.2.weight", "value_net.weight"]),
                   w(["mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.bias", "value_net.bias"]), "tanh")
    return a, c


def random_nets(seed=5):
    """A second member: dense random networks with log_std in [-1.4, -0.4] (a zero or symmetric log_std hides nothing)."""
    a = M.dense([64, 64], "tanh", seed=seed)
    a["log_std"] = np.random.default_rng([seed, 77]).uniform(-1.4, -0.4, size=6).astype(np.float32)
    return a, M.critic_of(M.dense([64, 64], "tanh", seed=seed + 1))


def clamp_nets():
    """A third member for the +-63 observation clamp: the random nets with column CLAMP_COL of both first-layer matrices times 2^-7, so
    that an input of 63 moves a pre-activation by about 0.5 w and tanh stays live (with ordinary weights such a row saturates and drops
    out of dW1 whatever the backward pass does with its input)."""
    actor, critic = random_nets()
    for net in (actor, critic):
        w1 = net["w"][0].copy()
        w1[:, CLAMP_COL] *= np.float32(2.0 ** -7)
        net["w"][0] = w1
    return actor, critic


MEMBERS = {"golden": golden_nets, "random": random_nets, "clamp": clamp_nets}
BASE_MEMBERS = ("golden", "random")                  # the members of the accuracy table; "clamp" has tests of its own
_STREAM = {"golden": 0, "random": 1, "clamp": 2}     # the member's random stream (fixed: the default cases keep their bits)


@functools.lru_cache(maxsize=None)
def make_case(member, seed=3, rows=ROWS):
    """The rows of the GPU test for one member, computed once and shared: dict(actor, critic, obs, actions, old_log_prob, advantages,
    returns) of ``rows`` float32 rows.  obs uniform in the Box, actions = mu64 + sigma z, advantages and returns N(0, 1),
    old_log_prob = log_prob64 - u with u uniform in [-0.6, 0.6]; rows whose fp64 ratio lies within GUARD of a clip limit get a new u
    (deterministically) until none does: otherwise a last-bit difference in log_prob flips a row's class.  The "clamp" member's
    rows 0, CLAMP_EVERY, 2 CLAMP_EVERY, ... carry CLAMP_VALUES, cyclically, in feature CLAMP_COL."""
    actor, critic = MEMBERS[member]()
    rng = np.random.default_rng([seed, _STREAM[member]])
    obs = rng.uniform(-1.0, 1.0, size=(rows, 17)).astype(np.float32)
    if member == "clamp":
        at = np.arange(0, rows, CLAMP_EVERY)
        obs[at, CLAMP_COL] = np.asarray(CLAMP_VALUES, np.float32)[np.arange(at.size) % len(CLAMP_VALUES)]
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
                advantages=rng.standard_normal(rows).astype(np.float32), returns=rng.standard_normal(rows).astype(np.float32))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def big_case(member):
    """The BIG_ROWS-row case of a member, by the recipe of the default one (the large minibatches of the GPU test)."""
    return make_case(member, rows=BIG_ROWS)


def repeated_index_vector(base=REPEAT_BASE, times=REPEAT_TIMES, seed=12):
    """Rows 0 .. base - 1, ``times`` times each, shuffled: the workgroups differ, and every sample has the same multiplicity, so that in
    exact arithmetic the loss, every gradient and every scalar are those of the minibatch of the first ``base`` rows."""
    return np.random.default_rng([seed, base, times]).permutation(np.tile(np.arange(base, dtype=np.int64), times))


# ------------------------------------------------------------------------------------------------------------ degenerate error tiles
def with_columns(case, **columns):
    """The case with some columns replaced (float32, read-only); the nets and the other columns are shared, not copied."""
    out = dict(case)
    for k, v in columns.items():
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.shape == case[k].shape, k
        v.setflags(write=False)
        out[k] = v
    return out


def zero_policy_gradient(case, mask=None):
    """The case with the rows of ``mask`` (all rows when None) on the zero-gradient side of the clip: old_log_prob = float32(lp64 - s / 2)
    and advantage = s |A| with s = +1 on even rows, -1 on odd ones.  The ratio is e^(+-1/2) = 1.65 / 0.61, far outside [1 - EPS, 1 + EPS],
    with the clipped term the smaller one, so d policy_loss / d log_prob of such a row is exactly zero."""
    rows = case["obs"].shape[0]
    mask = np.ones(rows, bool) if mask is None else np.asarray(mask, bool)
    lp = analytic64(case["actor"], case["critic"], *take(case, rows))["log_prob"]
    s = np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)
    old = np.where(mask, (lp - 0.5 * s).astype(np.float32), case["old_log_prob"])
    adv = np.where(mask, (s * np.abs(case["advantages"].astype(np.float64))).astype(np.float32), case["advantages"])
    return with_columns(case, old_log_prob=old, advantages=adv)


DEAD_N = 549


def dead_wave_mask(rows=ROWS):
    """n = DEAD_N (three workgroups; a wave owns 32 rows, a workgroup 256): waves 0, 2, 5 of workgroup 0 and the whole of workgroup 1
    have no policy gradient, and so has the last, partial wave (rows 512 .. 548) but for its last row."""
    mask = np.zeros(rows, bool)
    for wave in (0, 2, 5):
        mask[32 * wave:32 * wave + 32] = True
    mask[256:512] = True
    mask[512:DEAD_N - 1] = True
    return mask


def wide_advantages(case, seed=17):
    """The case with advantages sign 10^U(-6, 4): ten decades inside one wave."""
    rng = np.random.default_rng(seed)
    rows = case["obs"].shape[0]
    return with_columns(case, advantages=rng.choice([-1.0, 1.0], size=rows) * 10.0 ** rng.uniform(-6.0, 4.0, size=rows))


def with_nan(case, column, row=540, component=3):
    """The case with one NaN: ``column`` of ``row`` (component ``component`` of obs and actions)."""
    v = np.array(case[column])
    v[(row, component) if v.ndim == 2 else row] = np.nan
    return with_columns(case, **{column: v})


def nan_pattern(grads, scalars):
    """(names of the gradient tensors that are NaN in every entry, names of the NaN scalars); a tensor is all-NaN or finite throughout."""
    names = []
    for name, g in zip(NAMES, grads):
        bad = np.isnan(np.asarray(g))
        assert bad.all() or (not bad.any() and np.isfinite(np.asarray(g)).all()), name
        if bad.all():
            names.append(name)
    assert all(np.isnan(scalars[k]) or np.isfinite(scalars[k]) for k in SCALARS)
    return tuple(names), tuple(k for k in SCALARS if np.isnan(scalars[k]))


COLUMNS = ("obs", "actions", "old_log_prob", "advantages", "returns")
NAN_ROW = 540                                        # of n = 549: in the last, partial wave of the last workgroup
NAN_RULE = {                                         # rdv.h: a NaN in any sampled row reaches the gradients and the scalars — these ones
    "obs": (NAMES, ("loss", "policy_loss", "value_loss", "approx_kl")),
    "actions": (NAMES[:7], ("loss", "policy_loss", "approx_kl")),
    "old_log_prob": (NAMES[:7], ("loss", "policy_loss", "approx_kl")),
    "advantages": (NAMES[:7], ("loss", "policy_loss")),
    "returns": (NAMES[7:], ("loss", "value_loss")),
}


def index_vector(n, seed=9):
    """A shuffled index vector of n samples that contains duplicates (n >= 4) and reaches row 0 and row ROWS - 1 (n >= 2)."""
    rng = np.random.default_rng([seed, n])
    idx = rng.permutation(ROWS)[:n].astype(np.int64)
    if n >= 2:
        idx[0], idx[n - 1] = ROWS - 1, 0
    if n >= 4:
        idx[n // 2] = idx[1]
    return idx


def take(case, idx):
    """(obs, actions, old_log_prob, advantages, returns) of the minibatch: rows idx (an index vector) or the first idx rows (an int)."""
    sel = slice(0, idx) if isinstance(idx, (int, np.integer)) else idx
    return tuple(case[k][sel] for k in ("obs", "actions", "old_log_prob", "advantages", "returns"))


def class_shares(ratio, adv, eps=EPS):
    """Shares of the six classes {ratio below, inside, above the clip range} x {A < 0, A > 0}."""
    where = np.where(ratio < 1.0 - eps, 0, np.where(ratio > 1.0 + eps, 2, 1))
    return {(w, s): float(((where == w) & ((adv > 0) == bool(s))).mean()) for w in range(3) for s in range(2)}


# ------------------------------------------------------------------------------------------------------------ budgets
def mean_budget(actor, obs):
    """The fp32 budget of the actor's means that tests/test_gpu_policy_mlp.py asserts: 1.5 e32 + A (policy_mlp_reference.bounds)."""
    _, e32, a_entry = M.bounds(actor, R.clamp_obs(np.asarray(obs, np.float32)))
    return 1.5 * e32 + a_entry


def log_prob_budget(actor, obs, actions):
    """The means' budget propagated through the density, per row: |d log_prob / d mu_c| = |a_c - mu_c| / sigma_c^2 times the means'
    budget, plus the float32 evaluation of the expression itself — per component at most 8 roundings of 2^-24 on the term
    (a - mu, its square, sigma = float(exp(log_std)), sigma^2, 2 sigma^2, the quotient) and one per partial sum, the sums bounded by
    sum_c (t_c + |log_std_c|) + 3 ln 2 pi."""
    x = R.clamp_obs(np.asarray(obs, np.float32)).astype(np.float64)
    ls = actor["log_std"].astype(np.float64)
    var = np.exp(2.0 * ls)
    d = np.asarray(actions, np.float64) - _forward64(actor, x)[2]
    t = d ** 2 / (2.0 * var)
    size = (t + np.abs(ls)).sum(1) + 3.0 * LOG_2PI
    return (np.abs(d) / var).sum(1) * mean_budget(actor, obs) + 2.0 ** -24 * (8.0 * t.sum(1) + 8.0 * size)

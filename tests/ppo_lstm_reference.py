"""
Reference of the recurrent PPO minibatch loss and its gradients (include/rdv.h, "Recurrent PPO minibatch gradients"; csrc/rdv_ppo_lstm.h)
for the networks of tests/policy_lstm_reference.py: a minibatch of B whole env columns of a [T, N] rollout, each net's LSTM stepped one t
at a time from the constant ``state0`` with the ``(1 - s_t)`` masks (s_0 = 0: state0 is given as step 0 sees it; s_t = done[t-1]), the
trunk behind it, SB3's loss over the T B rows, differentiated by torch autograd:

  * ``reference(case, "float64")``: through ``torch.nn.LSTM`` and ``Linear`` modules in double — the reference G64;
  * ``reference(case, "float32")``: the same in float — the yardstick e32 of the accuracy rule, and the mathematics of
    ``LstmPolicy.ppo_sequence_grad``'s PyTorch fallback;
  * ``reference(case, dtype, wrong=...)``: the same loss over a cell written out (pinned to the module form by
    tests/test_ppo_lstm_grad.py) with ONE of four wrong restatements of the backward pass, the forward values unchanged:
      crosses_done        the gradient crosses an episode start (done[t-1] = 1 lets d h_t, d c_t into step t - 1)
      whh_unmasked        h_{t-1} is not masked in dW_hh at an episode start
      state0_zero         state0 is taken as zero (this one changes the forward pass too)
      dc_without_forget   d c_t is carried into d c_{t-1} without the forget gate
    The accuracy rule must tell each from the right one on the GPU cases' inputs.

``make_case(name)`` builds the cases of tests/test_gpu_ppo_lstm_grad.py (CASES): the smallest shapes at which each mechanism can go
wrong.  Runs on the CPU.
"""
import functools

import numpy as np
import torch

import policy_lstm_reference as L
import policy_mlp_reference as M
import policy_reference as R
from ppo_reference import EPS, GUARD, LOG_2PI, SCALARS, rel_err

WRONG = ("crosses_done", "whh_unmasked", "state0_zero", "dc_without_forget")
C_TENSOR, C_SCALAR = 32.0, 128.0       # the constants of rdv_ppo_mlp for the same operand precision (include/rdv.h)
FLOOR = 2.0 ** -23
PRE_GUARD = 1e-4                       # ReLU: no fp64 hidden pre-activation of a case within this of 0
ENT, VF = 0.01, 0.5

# name: (H, pi arch, vf arch, activation, weight class, T, N, B, done pattern, what it exercises)
CASES = {
    "h32_partial_wave": (32, [64, 64], [64, 64], "tanh", "hot", 5, 48, 33, "random"),          # random done, state0 of a second rollout, envs with a duplicate
    "h64_lone_row": (64, [32], [32], "relu", "hot", 3, 1, 1, "random"),
    "h128_two_workgroups": (128, [64, 64], [64, 64], "tanh", "hot", 2, 257, 257, "random"),   # the partial-sum order
    "h256_widest": (256, [16, 16], [16, 16], "sigmoid", "default_init", 4, 33, 33, "random"),
    "t1_no_recurrence": (32, [64, 64], [64, 64], "tanh", "default_init", 1, 256, 256, "random"),
    "long_memory": (32, [64, 64], [32, 16], "tanh", "long_memory", 32, 33, 33, "sparse"),
    "all_done": (32, [32, 16], [64], "tanh", "hot", 4, 33, 33, "all_done"),                    # a step where every column is done; a column done at every step
}
DEFECT_CASES = ("h32_partial_wave", "long_memory", "all_done")


def names(actor, critic):
    """The gradient tensors in the order of actor_grad, critic_grad (rdv_lstm_ppo_grad_floats)."""
    out = []
    for who, net in (("actor", actor), ("critic", critic)):
        out += [f"{who}.w_ih", f"{who}.w_hh", f"{who}.b_ih", f"{who}.b_hh"]
        for l in range(len(net["w"])):
            out += [f"{who}.w{l + 1}", f"{who}.b{l + 1}"]
        if who == "actor":
            out.append("actor.log_std")
    return tuple(out)


def shapes(net, actor):
    H = L.hidden_of(net)
    out = [(4 * H, 17), (4 * H, H), (4 * H,), (4 * H,)]
    for w in net["w"]:
        out += [tuple(w.shape), (w.shape[0],)]
    return out + ([(6,)] if actor else [])


def split_flat(flat, net, actor):
    """A flat gradient buffer -> its tensors (float64 arrays)."""
    flat = np.asarray(flat, np.float64)
    out, at = [], 0
    for s in shapes(net, actor):
        k = int(np.prod(s))
        out.append(flat[at:at + k].reshape(s)); at += k
    assert at == flat.size, (at, flat.size)
    return out


# ------------------------------------------------------------------------------------------------------------ the networks in torch
def _act(name, z):
    if name == "tanh":
        return torch.tanh(z)
    if name == "sigmoid":
        return torch.sigmoid(z)
    h = torch.relu(z)
    return torch.where(h < M.RELU_CLAMP, h, torch.full_like(h, M.RELU_CLAMP))


class _Net:
    """torch.nn.LSTM(17, H) and the trunk's Linear layers of one net dict, in ``dt``."""

    def __init__(self, net, dt):
        t = lambda a: torch.as_tensor(np.array(a, np.float32)).to(dt)
        H = L.hidden_of(net)
        self.H, self.act = H, net["act"]
        self.lstm = torch.nn.LSTM(17, H, num_layers=1).to(dt)
        with torch.no_grad():
            for k, a in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
                getattr(self.lstm, k).copy_(t(net[a]))
        self.lins = []
        for w, b in zip(net["w"], net["b"]):
            lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dt)
            with torch.no_grad():
                lin.weight.copy_(t(w)); lin.bias.copy_(t(b))
            self.lins.append(lin)

    def params(self):
        return [self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0, self.lstm.bias_hh_l0] + \
            [p for lin in self.lins for p in (lin.weight, lin.bias)]

    def trunk(self, x):
        for lin in self.lins[:-1]:
            x = _act(self.act, lin(x))
        return self.lins[-1](x)

    def latents(self, x, start, h0, c0, wrong=None, written_out=False):
        """h_t [T, B, H] from clamped rows x [T, B, 17], start [T, B] (row 0 zeros) and the constant state0."""
        if wrong == "state0_zero":
            h0, c0 = torch.zeros_like(h0), torch.zeros_like(c0)
        h, c, out = h0, c0, []
        for t in range(x.shape[0]):
            keep = (1.0 - start[t])[:, None]
            if wrong is None and not written_out:
                _, (h1, c1) = self.lstm(x[t][None], ((h * keep)[None], (c * keep)[None]))
                h, c = h1[0], c1[0]
            else:
                h, c = self._cell(x[t], h, c, keep, wrong)
            out.append(h)
        return torch.stack(out)

    def _cell(self, x, h, c, keep, wrong):
        """The cell written out; ``wrong`` changes what flows backward and nothing of the values."""
        W_ih, W_hh, b_ih, b_hh = self.params()[:4]
        h_in, c_in = h * keep, c * keep
        if wrong == "crosses_done":                                   # value (1 - s) h, derivative 1
            h_in = h_in + (h - h.detach()) * (1.0 - keep)
            c_in = c_in + (c - c.detach()) * (1.0 - keep)
        a = x @ W_ih.T + b_ih + h_in @ W_hh.T + b_hh
        if wrong == "whh_unmasked":                                   # value 0; dW_hh gains da^T (s h_{t-1})
            cut = (h * (1.0 - keep)).detach()
            a = a + cut @ W_hh.T - cut @ W_hh.detach().T
        i, f, g, o = a.chunk(4, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        fc = f * c_in
        if wrong == "dc_without_forget":                              # value f c; d / dc = 1, d / df = c
            fc = fc.detach() + (c_in - c_in.detach()) + (f - f.detach()) * c_in.detach()
        c1 = fc + i * g
        return o * torch.tanh(c1), c1


def minibatch(case):
    """The gathered columns of a case: dict(obs [T,B,17], actions [T,B,6], old_log_prob, advantages, returns [T,B], start [T,B] float,
    actor_state0, critic_state0: pairs of [B,H]) as float32 / float64 arrays."""
    e = case["envs"] if case["envs"] is not None else np.arange(case["N"])
    done = case["done"]
    start = np.concatenate([np.zeros_like(done[:1]), done[:-1]], axis=0)[:, e].astype(np.float64)
    mb = {k: case[k][:, e] for k in ("obs", "actions", "old_log_prob", "advantages", "returns")}
    mb["start"] = start
    mb["actor_state0"] = tuple(a[e] for a in case["actor_state0"])
    mb["critic_state0"] = tuple(a[e] for a in case["critic_state0"])
    return mb


def reference(case, dtype="float64", wrong=None, written_out=False, eps=EPS, ent_coef=ENT, vf_coef=VF, mb=None):
    """dict(grads=[float64 arrays in ``names`` order], scalars={name: float}, log_prob [T,B], values [T,B], pre=(hidden pre-activation
    magnitudes are not kept)) of the minibatch ``mb`` (default: ``minibatch(case)``) by autograd in ``dtype``."""
    dt = getattr(torch, dtype)
    t = lambda a: torch.as_tensor(np.array(a, np.float32)).to(dt)
    mb = minibatch(case) if mb is None else mb
    T, B = mb["obs"].shape[:2]
    actor, critic = _Net(case["actor"], dt), _Net(case["critic"], dt)
    log_std = torch.nn.Parameter(t(case["actor"]["log_std"]))
    x = t(R.clamp_obs(np.asarray(mb["obs"], np.float32).reshape(T * B, 17)).reshape(T, B, 17))
    start = torch.as_tensor(mb["start"]).to(dt)
    lat_a = actor.latents(x, start, *[t(a) for a in mb["actor_state0"]], wrong=wrong, written_out=written_out)
    lat_c = critic.latents(x, start, *[t(a) for a in mb["critic_state0"]], wrong=wrong, written_out=written_out)
    mean = actor.trunk(lat_a).reshape(T * B, 6)
    values = critic.trunk(lat_c).reshape(T * B)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp(), validate_args=False)
    log_prob, entropy = dist.log_prob(t(mb["actions"]).reshape(T * B, 6)).sum(dim=1), dist.entropy().sum(dim=1)
    adv, old, ret = (t(mb[k]).reshape(T * B) for k in ("advantages", "old_log_prob", "returns"))
    ratio = torch.exp(log_prob - old)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - eps, 1 + eps)).mean()
    value_loss = torch.nn.functional.mse_loss(ret, values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    grads = torch.autograd.grad(loss, actor.params() + [log_std] + critic.params())
    with torch.no_grad():
        log_ratio = log_prob - old
        approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        clip_fraction = torch.mean((torch.abs(ratio - 1) > eps).to(dt))
    scalars = dict(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, approx_kl=approx_kl, clip_fraction=clip_fraction)
    return dict(grads=[g.detach().to(torch.float64).numpy() for g in grads], scalars={k: float(v.detach()) for k, v in scalars.items()},
                log_prob=log_prob.detach().to(torch.float64).numpy().reshape(T, B), values=values.detach().to(torch.float64).numpy().reshape(T, B),
                ratio=ratio.detach().to(torch.float64).numpy())


# ------------------------------------------------------------------------------------------------------------ the accuracy rule
def tensor_err(g, w):
    """max|g - w| / max|w|; a reference tensor of zeros asks for zeros, by equality."""
    if not np.any(np.asarray(w)):
        return 0.0 if not np.any(np.asarray(g)) else float("inf")
    return rel_err(g, w)


def compare(tensor_names, got_grads, got_scalars, ref64, ref32):
    """rows (name, err, e32, C): every gradient tensor and five scalars against the fp64 reference, beside the float32 autograd yardstick."""
    rows = [(name, tensor_err(g, w), tensor_err(y, w), C_TENSOR) for name, g, w, y in zip(tensor_names, got_grads, ref64["grads"], ref32["grads"])]
    for name in SCALARS:
        if name != "clip_fraction":
            w = ref64["scalars"][name]
            rows.append((name, abs(got_scalars[name] - w) / abs(w), abs(ref32["scalars"][name] - w) / abs(w), C_SCALAR))
    return rows


def violations(rows):
    """The rows that break err <= C max(e32, 2^-23)."""
    return [(name, err, e32) for name, err, e32, C in rows if not err <= C * max(e32, FLOOR)]


# ------------------------------------------------------------------------------------------------------------ inputs
def _nets(H, pi, vf, act, cls, seed=5):
    make = L.ALL_CLASSES[cls]
    a = make(H, tuple(pi), act, seed=seed)
    a["log_std"] = np.random.default_rng([seed, 77]).uniform(-1.4, -0.4, size=6).astype(np.float32)
    return a, L.critic_of(make(H, tuple(vf), act, seed=seed + 1))


def _done(pattern, rng, T, N):
    if pattern == "all_done":
        d = (rng.uniform(size=(T, N)) < 0.2).astype(np.uint8)
        d[1, :] = 1                         # a step at which every column is done
        d[:, min(7, N - 1)] = 1             # a column done at every step
        return d
    p = 0.25 if pattern == "random" else 0.04
    return (rng.uniform(size=(T, N)) < p).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def make_case(name, seed=3):
    """One entry of CASES, computed once and shared: dict(actor, critic, H, T, N, B, envs (int64 [B] or None), obs [T,N,17], actions
    [T,N,6], old_log_prob, advantages, returns [T,N] float32, done [T,N] uint8, actor_state0, critic_state0: pairs of [N,H] float32).
    obs uniform in the Box; state0: the state a rollout of four steps of the same nets on other observations left, zero where an episode
    start is pending (a quarter of the columns) — non-zero elsewhere; actions = mu64 + sigma z; advantages and returns N(0, 1);
    old_log_prob = log_prob64 - u, u uniform in [-0.6, 0.6], redrawn while a row's fp64 ratio lies within GUARD of a clip limit.  N > B:
    ``envs`` is a permutation's first B - 1 columns and one of them again."""
    H, pi, vf, act, cls, T, N, B, pattern = CASES[name]
    actor, critic = _nets(H, pi, vf, act, cls)
    rng = np.random.default_rng([seed, sorted(CASES).index(name)])
    obs = rng.uniform(-1.0, 1.0, size=(T, N, 17)).astype(np.float32)
    done = _done(pattern, rng, T, N)
    envs = None
    if N > B:
        perm = rng.permutation(N)[:B - 1]
        envs = np.concatenate([perm, perm[3:4]]).astype(np.int64)
    pending = rng.uniform(size=N) < 0.25
    states = []
    for net in (actor, critic):
        with torch.no_grad():
            m = _Net(net, torch.float64)
            warm = torch.as_tensor(rng.uniform(-1.0, 1.0, size=(4, N, 17)))
            z = torch.zeros((N, H), dtype=torch.float64)
            h, c = z, z
            for t in range(4):
                _, (h1, c1) = m.lstm(warm[t][None], (h[None], c[None]))
                h, c = h1[0], c1[0]
        keep = (~pending)[:, None].astype(np.float32)
        states.append((h.numpy().astype(np.float32) * keep, c.numpy().astype(np.float32) * keep))
    case = dict(name=name, actor=actor, critic=critic, H=H, T=T, N=N, B=B, envs=envs, obs=obs, done=done, actor_state0=states[0], critic_state0=states[1],
                actions=np.zeros((T, N, 6), np.float32), old_log_prob=np.zeros((T, N), np.float32),
                advantages=rng.standard_normal((T, N)).astype(np.float32), returns=rng.standard_normal((T, N)).astype(np.float32))
    # the current policy's means over ALL columns, in fp64
    full = dict(case, envs=None)
    with torch.no_grad():
        dt = torch.float64
        a = _Net(actor, dt)
        mbf = minibatch(full)
        x = torch.as_tensor(R.clamp_obs(obs.reshape(T * N, 17)).reshape(T, N, 17)).to(dt)
        lat = a.latents(x, torch.as_tensor(mbf["start"]), *[torch.as_tensor(s).to(dt) for s in mbf["actor_state0"]])
        mu = a.trunk(lat).numpy()
        if act == "relu":
            for net, st in ((a, mbf["actor_state0"]), (_Net(critic, dt), mbf["critic_state0"])):
                hcur = net.latents(x, torch.as_tensor(mbf["start"]), *[torch.as_tensor(s).to(dt) for s in st])
                for lin in net.lins[:-1]:
                    z = lin(hcur)
                    assert float(z.abs().min()) > PRE_GUARD, (name, float(z.abs().min()))
                    hcur = _act(act, z)
    ls = actor["log_std"].astype(np.float64)
    case["actions"] = (mu + np.exp(ls) * rng.standard_normal((T, N, 6))).astype(np.float32)
    lp = (-((case["actions"].astype(np.float64) - mu) ** 2) / (2.0 * np.exp(2.0 * ls)) - ls - 0.5 * LOG_2PI).sum(-1)
    u = rng.uniform(-0.6, 0.6, size=(T, N))
    for _ in range(100):
        old = (lp - u).astype(np.float32)
        ratio = np.exp(lp - old.astype(np.float64))
        bad = (np.abs(ratio - (1.0 - EPS)) < GUARD) | (np.abs(ratio - (1.0 + EPS)) < GUARD)
        if not bad.any():
            break
        u[bad] = rng.uniform(-0.6, 0.6, size=int(bad.sum()))
    assert not bad.any()
    case["old_log_prob"] = old
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def references(name):
    """(fp64 reference, float32 yardstick) of a case, computed once and shared."""
    c = make_case(name)
    return reference(c, "float64"), reference(c, "float32")

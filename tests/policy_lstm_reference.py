"""
NumPy reference of the recurrent policy (csrc/rdv_policy_lstm.h; "The recurrent policy" in include/rdv.h): sb3-contrib's
RecurrentActorCriticPolicy with one LSTM layer and separate actor / critic LSTMs, restated per env row

    h, c   <- (1 - s) h, (1 - s) c
    a      =  W_ih x + b_ih + W_hh h + b_hh             gate order i, f, g, o (torch.nn.LSTM)
    c'     =  sigmoid(a_f) c + sigmoid(a_i) tanh(a_g);   h' = sigmoid(a_o) tanh(c')
    out    =  head(trunk(h'))

in float64 and in plain float32, the network classes, the defect restatements, the routing probes and the error budget that
tests/test_gpu_policy_lstm.py asserts.  The trunk, its activations and their constants are tests/policy_mlp_reference.py's.  Runs on
the CPU; pinned against torch.nn.LSTM by tests/test_policy_lstm.py.
"""
import numpy as np

import policy_mlp_reference as M
import policy_reference as R
from policy_reference import IN, OUT, SUBNORMAL_ABS_ERR, TANH_ABS_ERR

SIGMOID_ABS_ERR = M.SIGMOID_ABS_ERR
HIDDEN_SIZES = (32, 64, 128, 256)
BATCH_SIZES = M.BATCH_SIZES                       # (1, 31, 32, 33, 255, 256, 257, 1000)
T_STEPS = 6
DEFECTS = ("gate_order_ifog", "no_reset", "no_b_hh", "c_is_h")
EXTRA_TRUNKS = (([16], "relu"), ([32, 32, 32], "sigmoid"), ([64, 64, 64, 64], "tanh"))


# ------------------------------------------------------------------------------------------------------------ the network
def make_net(w_ih, w_hh, b_ih, b_hh, ws, bs, act="tanh", log_std=None):
    """dict(w_ih [4H,17], w_hh [4H,H], b_ih, b_hh [4H], w=[trunk layers, head], b=[...], act, log_std): float32, torch's layout."""
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    net = dict(w_ih=f(w_ih), w_hh=f(w_hh), b_ih=f(b_ih), b_hh=f(b_hh), w=[f(w) for w in ws], b=[f(b) for b in bs], act=act)
    H = net["w_hh"].shape[1]
    net["log_std"] = f(np.zeros(net["w"][-1].shape[0]) if log_std is None else log_std)
    assert net["w_ih"].shape == (4 * H, IN) and net["w_hh"].shape == (4 * H, H) and net["b_ih"].shape == net["b_hh"].shape == (4 * H,)
    assert net["w"][0].shape[1] == H and act in M.ACTS
    return net


def hidden_of(net):
    return int(net["w_hh"].shape[1])


def critic_of(net):
    """The out_dim = 1 network with the same LSTM and trunk: the first head row."""
    return make_net(net["w_ih"], net["w_hh"], net["b_ih"], net["b_hh"], net["w"][:-1] + [net["w"][-1][:1]], net["b"][:-1] + [net["b"][-1][:1]],
                    net["act"])


def weights_dict(actor, critic):
    """sb3-contrib's state-dict keys: what LstmPolicy infers H and the trunks from."""
    out = {"log_std": actor["log_std"]}
    for lstm, trunk, head, nn in (("lstm_actor", "policy_net", "action_net", actor), ("lstm_critic", "value_net", "value_net", critic)):
        for k, a in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            out[f"{lstm}.{k}"] = nn[a]
        for l, (w, b) in enumerate(zip(nn["w"][:-1], nn["b"][:-1])):
            out[f"mlp_extractor.{trunk}.{2 * l}.weight"], out[f"mlp_extractor.{trunk}.{2 * l}.bias"] = w, b
        out[f"{head}.weight"], out[f"{head}.bias"] = nn["w"][-1], nn["b"][-1]
    return out


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-x))).astype(x.dtype)


def cell(net, x, h, c, s, dt, defect=None, parts=None):
    """One step in dtype dt.  x [n,17] (clamped by the caller), h, c [n,H], s [n] in {0, 1} -> (h', c').  `defect`: one of DEFECTS,
    the wrong restatements the budget must tell apart.  `parts`, a dict, receives the gates and the reset c."""
    H = hidden_of(net)
    p = {k: net[k].astype(dt) for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    keep = (1 - np.asarray(s)).astype(dt)[:, None]
    if defect != "no_reset":
        h, c = h * keep, c * keep
    a = x.astype(dt) @ p["w_ih"].T + p["b_ih"] + h @ p["w_hh"].T
    if defect != "no_b_hh":
        a = a + p["b_hh"]
    order = (0, 1, 3, 2) if defect == "gate_order_ifog" else (0, 1, 2, 3)
    ai, af, ag, ao = (a[:, q * H:(q + 1) * H] for q in order)
    i, f, g, o = _sigmoid(ai), _sigmoid(af), np.tanh(ag), _sigmoid(ao)
    c1 = f * (h if defect == "c_is_h" else c) + i * g
    h1 = o * np.tanh(c1)
    assert h1.dtype == dt and c1.dtype == dt
    if parts is not None:
        parts.update(i=i, f=f, g=g, o=o, c=c, c1=c1)
    return h1, c1


def trunk(net, h, dt):
    x = h
    for w, b in zip(net["w"][:-1], net["b"][:-1]):
        x = M.activation(net["act"], x @ w.astype(dt).T + b.astype(dt))
    return x @ net["w"][-1].astype(dt).T + net["b"][-1].astype(dt)


def run(net, obs_seq, starts, dt=np.float64, defect=None, h0=None, c0=None):
    """T steps from the zero state (or h0, c0): (out [T,n,out_dim], h [T,n,H], c [T,n,H]) after every step, in dtype dt."""
    T, n = obs_seq.shape[:2]
    H = hidden_of(net)
    h = np.zeros((n, H), dt) if h0 is None else np.asarray(h0, dt)
    c = np.zeros((n, H), dt) if c0 is None else np.asarray(c0, dt)
    outs, hs, cs = [], [], []
    for t in range(T):
        h, c = cell(net, R.clamp_obs(np.asarray(obs_seq[t], np.float32)), h, c, starts[t], dt, defect)
        outs.append(trunk(net, h, dt)); hs.append(h); cs.append(c)
    return np.stack(outs), np.stack(hs), np.stack(cs)


# -------------------------------------------------------------------------------------------------------------- the budget
def budget(net, obs_seq, starts):
    """The first-order, entrywise error budget of the kernel, on the float64 reference's own values:

        d_a  = |W_hh| d_h                                       (d_h = d_c = 0 where an episode starts, and before step 0)
        d_i, d_f, d_o = D_sigmoid + d_a / 4;   d_g = D_tanh + d_a
        d_c' = d_f |c| + f d_c + d_i |tanh a_g| + i d_g
        d_h' = d_o |tanh c'| + o (D_tanh + d_c')
        trunk: a_0 = d_h', a_l = Lip (|W_l| a_{l-1}) + d_act + 6e-8, A = |W_head| a_L      (policy_mlp_reference.error_floor_entrywise)

    Returns dict(out64, h64, c64 [T,n,...] float64; e32_out, e32_h, e32_c [T,n] = max|float32 run - float64 run| per step and row;
    A_out, A_h, A_c [T,n] = the budget's maximum per step and row).  Rows are independent, so the budget of the first k rows is a slice.
    The asserted tolerance is 1.5 e32 + A, as in test_gpu_policy_mlp.py: tolerance()."""
    T, n = obs_seq.shape[:2]
    H = hidden_of(net)
    f8 = np.float64
    out64, h64, c64 = run(net, obs_seq, starts, f8)
    out32, h32, c32 = run(net, obs_seq, starts, np.float32)
    e = lambda a32, a64: np.abs(a32.astype(f8) - a64).max(axis=2)
    res = dict(out64=out64, h64=h64, c64=c64, e32_out=e(out32, out64), e32_h=e(h32, h64), e32_c=e(c32, c64))
    aw_hh = np.abs(net["w_hh"].astype(f8))
    d_h, d_c = np.zeros((n, H)), np.zeros((n, H))
    h, c = np.zeros((n, H)), np.zeros((n, H))
    A_out, A_h, A_c = [], [], []
    lip, d_act = M.LIP[net["act"]], M.D_ACT[net["act"]]
    for t in range(T):
        keep = (1 - np.asarray(starts[t])).astype(f8)[:, None]
        d_h, d_c = d_h * keep, d_c * keep
        parts = {}
        h, c = cell(net, R.clamp_obs(np.asarray(obs_seq[t], np.float32)), h, c, starts[t], f8, parts=parts)
        d_a = d_h @ aw_hh.T
        d_i, d_f, d_g, d_o = (SIGMOID_ABS_ERR + d_a[:, 0:H] / 4, SIGMOID_ABS_ERR + d_a[:, H:2 * H] / 4, TANH_ABS_ERR + d_a[:, 2 * H:3 * H],
                              SIGMOID_ABS_ERR + d_a[:, 3 * H:] / 4)
        d_c = d_f * np.abs(parts["c"]) + parts["f"] * d_c + d_i * np.abs(parts["g"]) + parts["i"] * d_g
        d_h = d_o * np.abs(np.tanh(parts["c1"])) + parts["o"] * (TANH_ABS_ERR + d_c)
        a = d_h
        for w in net["w"][:-1]:
            a = lip * (a @ np.abs(w.astype(f8)).T) + d_act + SUBNORMAL_ABS_ERR
        A_out.append((a @ np.abs(net["w"][-1].astype(f8)).T).max(axis=1)); A_h.append(d_h.max(axis=1)); A_c.append(d_c.max(axis=1))
    res.update(A_out=np.asarray(A_out), A_h=np.asarray(A_h), A_c=np.asarray(A_c))
    return res


def tolerance(bud, what, n=None):
    """[T]: 1.5 e32 + A of `what` in ("out", "h", "c") over the first n rows (None: all), e32 and A each at their maximum over those rows."""
    return 1.5 * bud[f"e32_{what}"][:, :n].max(axis=1) + bud[f"A_{what}"][:, :n].max(axis=1)


def defect_factor(net, obs_seq, starts, defect, bud=None):
    """By how much the wrong restatement `defect` leaves the budget: max over steps of |defect run - reference| / (1.5 e32 + A), outputs."""
    bud = budget(net, obs_seq, starts) if bud is None else bud
    out, _, _ = run(net, obs_seq, starts, np.float64, defect)
    T = out.shape[0]
    err = np.abs(out - bud["out64"]).reshape(T, -1).max(axis=1)
    return float((err / tolerance(bud, "out")).max())


# ------------------------------------------------------------------------------------------------------- network classes
def _trunk_layers(rng, H, arch, out_dim=OUT):
    """nn.Linear's default initialisation: weights and biases U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    d = [H] + list(arch) + [out_dim]
    ws, bs = [], []
    for l in range(len(d) - 1):
        k = 1.0 / np.sqrt(d[l])
        ws.append(rng.uniform(-k, k, size=(d[l + 1], d[l]))); bs.append(rng.uniform(-k, k, size=d[l + 1]))
    return ws, bs


def default_init(H, arch=(64, 64), act="tanh", seed=51):
    """torch's default initialisation of nn.LSTM(17, H): every LSTM parameter U(-1/sqrt(H), 1/sqrt(H)); the trunk's nn.Linear
    layers at theirs."""
    rng = np.random.default_rng([seed, H, M.ACTS.index(act)] + list(arch))
    k = 1.0 / np.sqrt(H)
    u = lambda *shape: rng.uniform(-k, k, size=shape)
    ws, bs = _trunk_layers(rng, H, arch)
    return make_net(u(4 * H, IN), u(4 * H, H), u(4 * H), u(4 * H), ws, bs, act)


def hot(H, arch=(64, 64), act="tanh", seed=51):
    """default_init with the LSTM weights times 3 and the forget-gate bias + 1: the recursion matters (with the default initialisation a
    float32 run of 64 steps at H = 256 stays within 3.8e-8 of float64 and would test nothing of it)."""
    net = default_init(H, arch, act, seed)
    b_ih = net["b_ih"].copy(); b_ih[H:2 * H] += 1.0
    return make_net(3.0 * net["w_ih"], 3.0 * net["w_hh"], b_ih, net["b_hh"], net["w"], net["b"], act)


CLASSES = {"default_init": default_init, "hot": hot}


def route_probe(H, m, seed=52):
    """One-path network number m: row u of gate q reads ONE input feature and ONE state unit,
        W_ih[q H + u, (u + 5 q + m) % 17] = +-0.9,   W_hh[q H + u, (7 u + 3 q + 37 m + 1) % H] = +-1.4
    (7 is coprime to H: a permutation of the units per gate), distinct biases on every row, and a trunk [32] whose unit v reads state
    units (5 v + m) % H and (11 v + 3 m + 7) % H.  A fragment of the wrong tile, k-step or lane puts another weight, or none, on the path."""
    rng = np.random.default_rng([seed, H, m])
    w_ih, w_hh = np.zeros((4 * H, IN)), np.zeros((4 * H, H))
    u = np.arange(H)
    for q in range(4):
        w_ih[q * H + u, (u + 5 * q + m) % IN] = 0.9 * rng.choice([-1.0, 1.0], size=H)
        w_hh[q * H + u, (7 * u + 3 * q + 37 * m + 1) % H] = 1.4 * rng.choice([-1.0, 1.0], size=H)
    b_ih, b_hh = rng.permutation(np.linspace(-0.5, 0.5, 4 * H)), rng.permutation(np.linspace(-0.3, 0.3, 4 * H))
    v = np.arange(32)
    w1 = np.zeros((32, H)); w1[v, (5 * v + m) % H] = 0.8; w1[v, (11 * v + 3 * m + 7) % H] += -0.6
    w2 = np.zeros((OUT, 32)); w2[np.arange(32) % OUT, v] = rng.uniform(0.1, 0.3, size=32) * rng.choice([-1.0, 1.0], size=32)
    return make_net(w_ih, w_hh, b_ih, b_hh, [w1, w2], [rng.permutation(np.linspace(-0.4, 0.4, 32)), np.linspace(-0.1, 0.1, OUT)], "tanh")


def route_coverage(H, n_probes):
    """Share of the (gate, 32-row tile, 16-column k-step) fragments of W_hh that hold a non-zero weight in one of the probes."""
    seen = np.zeros((4 * H // 32, H // 16), bool)
    for m in range(n_probes):
        nz = route_probe(H, m)["w_hh"] != 0
        seen |= nz.reshape(4 * H // 32, 32, H // 16, 16).any(axis=(1, 3))
    return float(seen.mean())


ROUTE_PROBES = 3


# ------------------------------------------------------------------------------------------------------------ input sets
def obs_sequence(n, T=T_STEPS, seed=60):
    """[T, n, 17] distinct observation rows inside the Box, another set per step."""
    return np.stack([R.distinct_rows(n, seed=seed + t) for t in range(T)])


def episode_starts(n, T=T_STEPS):
    """[T, n] uint8: every row starts at step 0, rows 0, 3, 6, .. at step 2, rows 1, 6, 11, .. at step 3."""
    s = np.zeros((T, n), np.uint8)
    r = np.arange(n)
    s[0] = 1
    if T > 2:
        s[2] = r % 3 == 0
    if T > 3:
        s[3] = r % 5 == 1
    return s

"""
NumPy reference of the recurrent policy (csrc/rdv_policy_lstm.h; "The recurrent policy" in include/rdv.h): sb3-contrib's
RecurrentActorCriticPolicy with one LSTM layer and separate actor / critic LSTMs, restated per env row

    h, c   <- (1 - s) h, (1 - s) c
    a      =  W_ih x + b_ih + W_hh h + b_hh             gate order i, f, g, o (torch.nn.LSTM)
    c'     =  sigmoid(a_f) c + sigmoid(a_i) tanh(a_g);   h' = sigmoid(a_o) tanh(c')
    out    =  head(trunk(h'))

in float64 and in plain float32, the network classes, the defect restatements, the routing probes and the error budgets that
tests/test_gpu_policy_lstm.py asserts: budget() along a run from the zero state, local_budget() for ONE step from a given state.  Where
h enters the recurrent product, and nowhere else, it is clamped to +-63 (rdv.h; +-inf counts as +-63, as for an observation): no effect
on a state the cell produced.  The trunk, its activations and their constants are tests/policy_mlp_reference.py's.  Runs on the CPU;
pinned against torch.nn.LSTM by tests/test_policy_lstm.py.
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
# h_not_clamped: the state corners alone show it.  lo_term_dropped, shift_is_max: wrong restatements of the cell's weight quantisation.
QUANT_DEFECTS = ("lo_term_dropped", "shift_is_max")
H_CLAMP = 63.0                   # rdv.h: the state enters the matrix cores clamped to +-63
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


def clamp_h(h):
    """The state as the recurrent product reads it: clamped to +-63, NaN kept (np.clip keeps NaN)."""
    return np.clip(h, -H_CLAMP, H_CLAMP)


def cell_shift(net, defect=None):
    """rdv.h: W_ih and W_hh share ONE power-of-two scale, the smaller of their documented shifts."""
    s_ih, s_hh = R.documented_shift(net["w_ih"]), R.documented_shift(net["w_hh"])
    return max(s_ih, s_hh) if defect == "shift_is_max" else min(s_ih, s_hh)


def quantised(w, s, lo_term=True):
    """rdv_policy.h: w 2^s = hi + lo, hi = float16(w 2^s), lo = float16(w 2^s - hi) (the subtraction is exact in float32), both rounded
    to nearest even, subnormals kept -> (hi + lo) 2^-s in float64: the weight the matrix cores see.  |w| 2^s >= 65520 rounds to inf."""
    ws = np.ldexp(np.asarray(w, np.float32), s).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = ws.astype(np.float16)
        lo = (ws - hi.astype(np.float32)).astype(np.float16)
        q = hi.astype(np.float64) + (lo.astype(np.float64) if lo_term else 0.0)
    return np.ldexp(q, -s)


def cell_weights(net, defect=None):
    """(W_ih, W_hh) of the cell as quantised under the shared shift, float64; `defect` in QUANT_DEFECTS restates the rule wrongly."""
    s = cell_shift(net, defect)
    return tuple(quantised(net[k], s, lo_term=defect != "lo_term_dropped") for k in ("w_ih", "w_hh"))


def cell(net, x, h, c, s, dt, defect=None, parts=None):
    """One step in dtype dt.  x [n,17] (clamped by the caller), h, c [n,H], s [n] in {0, 1} -> (h', c').  `defect`: one of DEFECTS,
    "h_not_clamped" or QUANT_DEFECTS, the wrong restatements the budgets must tell apart.  `parts`, a dict, receives the gates, the
    reset c and the clamped h of the recurrent product."""
    H = hidden_of(net)
    p = {k: net[k].astype(dt) for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    if defect in QUANT_DEFECTS:
        p["w_ih"], p["w_hh"] = (w.astype(dt) for w in cell_weights(net, defect))
    h, c = np.asarray(h, dt), np.asarray(c, dt)
    if defect != "no_reset":
        keep = (np.asarray(s) == 0)[:, None]
        h, c = np.where(keep, h, dt(0)), np.where(keep, c, dt(0))          # (1 - s) h with 0 inf = 0: a started row reads no state
    hp = h if defect == "h_not_clamped" else clamp_h(h)
    with np.errstate(invalid="ignore", over="ignore"):
        a = x.astype(dt) @ p["w_ih"].T + p["b_ih"] + hp @ p["w_hh"].T
    if defect != "no_b_hh":
        a = a + p["b_hh"]
    order = (0, 1, 3, 2) if defect == "gate_order_ifog" else (0, 1, 2, 3)
    ai, af, ag, ao = (a[:, q * H:(q + 1) * H] for q in order)
    i, f, g, o = _sigmoid(ai), _sigmoid(af), np.tanh(ag), _sigmoid(ao)
    c1 = f * (h if defect == "c_is_h" else c) + i * g
    h1 = o * np.tanh(c1)
    assert h1.dtype == dt and c1.dtype == dt
    if parts is not None:
        parts.update(i=i, f=f, g=g, o=o, c=c, c1=c1, hp=hp)
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
    for t in range(T):
        keep = (1 - np.asarray(starts[t])).astype(f8)[:, None]
        d_h, d_c = d_h * keep, d_c * keep
        parts = {}
        h, c = cell(net, R.clamp_obs(np.asarray(obs_seq[t], np.float32)), h, c, starts[t], f8, parts=parts)
        d_h, d_c, a_out = _budget_step(net, parts, d_h @ aw_hh.T, d_c)
        A_out.append(a_out.max(axis=1)); A_h.append(d_h.max(axis=1)); A_c.append(d_c.max(axis=1))
    res.update(A_out=np.asarray(A_out), A_h=np.asarray(A_h), A_c=np.asarray(A_c))
    return res


def _budget_step(net, parts, d_a, d_c):
    """One step of budget()'s recursion from the error d_a of the pre-activations and d_c of the state read: (d_h', d_c', A of the outputs)."""
    H = hidden_of(net)
    f8 = np.float64
    d_i, d_f, d_g, d_o = (SIGMOID_ABS_ERR + d_a[:, 0:H] / 4, SIGMOID_ABS_ERR + d_a[:, H:2 * H] / 4, TANH_ABS_ERR + d_a[:, 2 * H:3 * H],
                          SIGMOID_ABS_ERR + d_a[:, 3 * H:] / 4)
    d_c = d_f * np.abs(parts["c"]) + parts["f"] * d_c + d_i * np.abs(parts["g"]) + parts["i"] * d_g
    d_h = d_o * np.abs(np.tanh(parts["c1"])) + parts["o"] * (TANH_ABS_ERR + d_c)
    lip, d_act = M.LIP[net["act"]], M.D_ACT[net["act"]]
    a = d_h
    for w in net["w"][:-1]:
        a = lip * (a @ np.abs(w.astype(f8)).T) + d_act + SUBNORMAL_ABS_ERR
    return d_h, d_c, a @ np.abs(net["w"][-1].astype(f8)).T


def local_budget(net, obs, starts, h0, c0):
    """The budget of ONE step from the state (h0, c0), float32 arrays [n, H] (exact in float64), observations [n, 17] and episode starts
    [n] (None: no row starts): budget()'s recursion taken for one step with d_h = d_c = 0 at its start, plus what the documented
    quantisation of the cell's weights leaves,

        d_a = |W_ih - Q(W_ih)| |x| + |W_hh - Q(W_hh)| |clamp(h)|        Q: quantised() under cell_shift(), computed exactly

    (with s_ih = s_hh = 10 the residual is 2^-22 |w| at most; when one matrix's outlier lowers the shared shift, the other's lo terms
    lose bits and this term carries the bound).  It does not grow with the number of steps before it: a check of every step along the
    device's own trajectory asserts the same thing at step 60 as at step 0.  Returns dict(out64 [n, out_dim], h64, c64 [n, H] float64;
    e32_out, e32_h, e32_c [n] = max|float32 step - float64 step| per row; A_out, A_h, A_c [n]).  Tolerance: local_tolerance()."""
    f8 = np.float64
    h0, c0 = np.asarray(h0, np.float32), np.asarray(c0, np.float32)
    n = h0.shape[0]
    s = np.zeros(n, np.uint8) if starts is None else np.asarray(starts)
    x = R.clamp_obs(np.asarray(obs, np.float32))
    parts = {}
    h64, c64 = cell(net, x, h0, c0, s, f8, parts=parts)
    h32, c32 = cell(net, x, h0, c0, s, np.float32)
    with np.errstate(invalid="ignore"):
        e = lambda a32, a64: np.abs(a32.astype(f8) - a64).max(axis=1)
        out64 = trunk(net, h64, f8)
        res = dict(out64=out64, h64=h64, c64=c64, e32_out=e(trunk(net, h32, np.float32), out64), e32_h=e(h32, h64), e32_c=e(c32, c64))
    q_ih, q_hh = cell_weights(net)
    d_a = np.abs(x.astype(f8)) @ np.abs(net["w_ih"].astype(f8) - q_ih).T + np.abs(parts["hp"]) @ np.abs(net["w_hh"].astype(f8) - q_hh).T
    d_h, d_c, a_out = _budget_step(net, parts, d_a, np.zeros_like(d_a[:, :hidden_of(net)]))
    res.update(A_out=a_out.max(axis=1), A_h=d_h.max(axis=1), A_c=d_c.max(axis=1))
    return res


def local_tolerance(bud, what, rows=None):
    """1.5 e32 + A of `what` in ("out", "h", "c") of a local_budget over `rows` (None: all), e32 and A each at their maximum over them."""
    rows = slice(None) if rows is None else rows
    return float(1.5 * bud[f"e32_{what}"][rows].max() + bud[f"A_{what}"][rows].max())


def local_defect_factor(net, obs, starts, h0, c0, defect, bud=None, rows=None):
    """By how much ONE step of the wrong restatement `defect` from (h0, c0) leaves the local tolerance: the largest of the three ratios
    |defect step - reference| / (1.5 e32 + A) of the outputs, h' and c' — the three comparisons the GPU tests make after every step (the
    trunk's own allowance hides from the outputs what h' shows).  A non-finite value (an unclamped inf, a weight scaled out of float16's
    range) counts as inf.  `rows`: the rows looked at (None: all).  Returns (factor, which of "out", "h", "c" gave it)."""
    bud = local_budget(net, obs, starts, h0, c0) if bud is None else bud
    s = np.zeros(len(obs), np.uint8) if starts is None else np.asarray(starts)
    h1, c1 = cell(net, R.clamp_obs(np.asarray(obs, np.float32)), np.asarray(h0, np.float32), np.asarray(c0, np.float32), s, np.float64, defect)
    best = (0.0, "")
    rows = slice(None) if rows is None else rows
    with np.errstate(invalid="ignore"):
        for what, got in (("out", trunk(net, h1, np.float64)), ("h", h1), ("c", c1)):
            err = np.abs(got - bud[f"{what}64"])[rows]
            best = max(best, (float(np.where(np.isfinite(err), err, np.inf).max() / local_tolerance(bud, what, rows)), what))
    return best


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


def _with_cell(net, **cell_arrays):
    p = dict(net, **cell_arrays)
    return make_net(p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"], p["w"], p["b"], p["act"])


def _outliers(w, rng, count, lo, hi, signed):
    """`count` entries of w, each in a row and a column of its own, set to U[lo, hi) (times +-1 when signed)."""
    w = w.copy()
    rows, cols = rng.choice(w.shape[0], count, replace=False), rng.choice(w.shape[1], count, replace=False)
    w[rows, cols] = rng.uniform(lo, hi, count) * (rng.choice([-1.0, 1.0], count) if signed else 1.0)
    return w


def hh_shift9(H, arch=(64, 64), act="tanh", seed=51):
    """hot with eight entries of W_hh at +-[33, 60): s_hh = 9 < s_ih = 10, the cell's shift is W_hh's."""
    net = hot(H, arch, act, seed)
    return _with_cell(net, w_hh=_outliers(net["w_hh"], np.random.default_rng([seed, H, 9]), 8, 33.0, 60.0, True))


def ih_shift3(H, arch=(64, 64), act="tanh", seed=51):
    """hot with four entries of W_ih at 3000: s_ih = 3 < s_hh = 10, the min takes the other side."""
    net = hot(H, arch, act, seed)
    return _with_cell(net, w_ih=_outliers(net["w_ih"], np.random.default_rng([seed, H, 3]), 4, 3000.0, 3000.0, False))


def hh_shift3(H, arch=(64, 64), act="tanh", seed=51):
    """hot with four entries of W_hh at 3000: s_hh = 3, and W_ih's lo terms lose bits under it (local_budget's residual term)."""
    net = hot(H, arch, act, seed)
    return _with_cell(net, w_hh=_outliers(net["w_hh"], np.random.default_rng([seed, H, 33]), 4, 3000.0, 3000.0, False))


def big_bias(H, arch=(64, 64), act="tanh", seed=51):
    """hot with b_ih shifted by U(-30, 30) on half of the 4H rows: gates exactly 0 and 1 beside live ones; |c| grows by up to 1 a step."""
    net = hot(H, arch, act, seed)
    rng = np.random.default_rng([seed, H, 30])
    b_ih = net["b_ih"].copy()
    rows = rng.choice(4 * H, 2 * H, replace=False)
    b_ih[rows] += rng.uniform(-30.0, 30.0, 2 * H)
    return _with_cell(net, b_ih=b_ih)


def long_memory(H, arch=(64, 64), act="tanh", seed=51):
    """default_init with W_hh times 0.25, W_ih times 3 and the forget-gate bias + 3: c integrates its inputs over about 20 steps."""
    net = default_init(H, arch, act, seed)
    b_ih = net["b_ih"].copy(); b_ih[H:2 * H] += 3.0
    return _with_cell(net, w_ih=3.0 * net["w_ih"], w_hh=0.25 * net["w_hh"], b_ih=b_ih)


# the classes of the scaling and state corners: the shifts (s_ih, s_hh) each is built to have
NEW_CLASSES = {"hh_shift9": hh_shift9, "ih_shift3": ih_shift3, "hh_shift3": hh_shift3, "big_bias": big_bias, "long_memory": long_memory}
CLASS_SHIFTS = {"default_init": (10, 10), "hot": (10, 10), "hh_shift9": (10, 9), "ih_shift3": (3, 10), "hh_shift3": (10, 3), "big_bias": (10, 10),
                "long_memory": (10, 10)}
ALL_CLASSES = dict(CLASSES, **NEW_CLASSES)


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


FAR_T = 48


def far_state(net, n):
    """(the observations of step FAR_T, the state (h, c) a float32 run of FAR_T steps from zero reaches in front of it): where big_bias has
    |c| near 48 and long_memory has integrated its inputs — states the six-step runs never see."""
    obs, starts = obs_sequence(n, FAR_T + 1), episode_starts(n, FAR_T + 1)
    _, hs, cs = run(net, obs[:FAR_T], starts[:FAR_T], np.float32)
    return obs[FAR_T], hs[-1], cs[-1]


H_CORNERS = (0.999, 1.0, -1.0, 5.0, -5.0, 62.9, -62.9, 63.0, -63.0, 64.0, -64.0, 1e3, -1e3, np.inf, -np.inf, -0.0)
C_CORNERS = (50.0, -50.0, 1e4, -1e4, 1e30, -1e30, 1e-30, -0.0)


def state_corners(net, n=33):
    """States that only rdv_lstm_set_state can put there.  The ordinary state is what a float32 run of T_STEPS steps reaches.  Rows 0, 4,
    8, .. keep it; each other row r takes one corner value (H_CORNERS in h, then C_CORNERS in c, in row order) on its units u with
    (u + r) % 4 == 0 and the ordinary state on the rest, so that a corner row's gates are not all saturated.  c stays finite.
    Returns dict(obs [n, 17], h_ord, c_ord, h, c [n, H] float32, ordinary = the rows that keep the ordinary state, kind[r] = "h=63", ..)."""
    H = hidden_of(net)
    assert n == 1 + 4 * ((len(H_CORNERS) + len(C_CORNERS)) // 3)
    _, hs, cs = run(net, obs_sequence(n), episode_starts(n), np.float32)
    h_ord, c_ord = hs[-1], cs[-1]
    h, c = h_ord.copy(), c_ord.copy()
    corner_rows = [r for r in range(n) if r % 4]
    kind = {r: "ordinary" for r in range(n)}
    for r, (what, v) in zip(corner_rows, [("h", v) for v in H_CORNERS] + [("c", v) for v in C_CORNERS]):
        (h if what == "h" else c)[r, (np.arange(H) + r) % 4 == 0] = v
        kind[r] = f"{what}={v:g}"
    return dict(obs=obs_sequence(n, 1, seed=75)[0], h_ord=h_ord, c_ord=c_ord, h=h, c=c, ordinary=[r for r in range(n) if r % 4 == 0], kind=kind)


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

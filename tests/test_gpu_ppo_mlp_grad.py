"""
GPU: rdv_ppo_mlp_loss_grad (include/rdv.h, "PPO minibatch gradients for every MLP architecture"; csrc/rdv_ppo_mlp.h) and MlpPolicy.ppo_grad
of other architectures than the shipped one against the fp64 reference of tests/ppo_mlp_reference.py.

Inputs (ppo_mlp_reference.make_case, the recipe of ppo_reference.make_case with policy_mlp_reference.dense networks): 1,200 rows, eps = 0.25,
no fp64 ratio within 1e-4 of a clip limit and, for ReLU, no fp64 hidden pre-activation within 1e-4 of 0 (asserted on the CPU in
tests/test_ppo_mlp_grad.py, with the other conditions).  Architectures (ppo_mlp_reference.CASES): the smallest set that reaches every hidden
(tiles, k-steps) shape, every head k-step count and depths 1..4 with tanh; [32, 16], [16, 64] and [64] x 4 with ReLU and sigmoid too;
pi = [32, 32], vf = [64, 16] ReLU (actor != critic); [64, 64] ReLU.  Shapes n in {1, 33, 257, 549}: a lone lane, a wave's edge, a 256-row
workgroup's edge, three workgroups with a 37-row last wave; for the 4 x 64 blocks, whose workgroups have four waves (128 rows), also
n in {127, 128, 129}.  Each with rows in order and with a shuffled index vector that holds duplicates and reaches rows 0 and 1199.

The accuracy rule is that of tests/test_gpu_ppo_grad.py, per gradient tensor and for five of the scalars:
    err = max|G_gpu - G64| / max|G64|  <=  C max(e32, 2^-23),
e32 the same quantity for PyTorch's float32 autograd of the same loss on the same minibatch (CPU).  C is the smallest power of two at
least twice the largest err / max(e32, 2^-23) of profiles/ppo_mlp_grad_accuracy.csv (tools/ppo_mlp_grad_accuracy.py), separately for
gradient tensors and scalars:
  * over the gradient tensors the largest ratio is 8.47 (actor.log_std of [16, 64] tanh, n = 1, rows in order: err 1.01e-6, e32 1.16e-7):
    C_GRAD = 32.  The cause is the FORWARD pass, not a backward product: with one sample every actor gradient is a multiple of
    ratio = exp(log_prob - old_log_prob), so the sample's log_prob error — 1.33e-6 here, the policy_loss row of the same call (-A ratio for
    a lone sample), inside the budget of assertion 1 — is the relative error of ALL seven actor tensors of that call (0.93e-6 .. 1.40e-6,
    ratios 3.5 .. 8.5; the critic's, which no ratio enters: 1.3 .. 2.9), while float32 autograd of that one sample happens to sit at
    1.2e-7 .. 2.7e-7.  With more than one sample the errors of
    the rows average: the largest ratio over n >= 33 is 5.37 (critic.b5 of 4 x 64 ReLU, n = 257), which alone would give 16, the shipped
    kernel's constant;
  * over the scalars it is 39.8 (policy_loss of [16, 16] sigmoid, n = 33, rows in order): C_BOUND = 128, as for the shipped kernel and
    for its reason (tests/test_gpu_ppo_grad.py: policy_loss and approx_kl are functions of log_prob alone and the noisy remainder of a
    cancellation over the rows; e32 of that row is 7.9e-8, below the floor).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_reference as M
import ppo_mlp_reference as Q
import ppo_reference as P
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd.policy import ACTIVATIONS, MlpPolicy, PolicySet
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# profiles/ppo_mlp_grad_accuracy.csv: the largest ratio of a gradient tensor and of a scalar, and the rows that set them
C_GRAD = 32.0      # 8.4746: 16x64,16x64,tanh,1,0,actor.log_std,1.0103e-06,1.1627e-07
C_BOUND = 128.0    # 39.8197: 16x16,16x16,sigmoid,33,0,policy_loss,4.7469e-06,7.8675e-08
FLOOR = 2.0 ** -23
ENT, VF = 0.01, 0.5


def make_policy(actor, critic):
    return MlpPolicy(M.weights_dict(actor, critic), activation_fn=actor["act"]).to(DEV)


def specs(actor, critic):
    return (N.MlpSpec.make(M.arch_of(actor), ACTIVATIONS[actor["act"]][0]), N.MlpSpec.make(M.arch_of(critic), ACTIVATIONS[critic["act"]][0]))


def device_columns(case):
    return {k: torch.from_numpy(np.array(case[k])).to(DEV) for k in P.COLUMNS}


def call(pol, nets, cols, n, idx=None, eps=P.EPS, ent=ENT, vf=VF, actor=None, critic=None, workspace=None, raw=False, fn="rdv_ppo_mlp_loss_grad"):
    """rdv_ppo_mlp_loss_grad on the current stream -> dict(grads [arrays in Q.names order], scalars, log_prob, values, raw) (or the return
    code and message with raw=True).  nets: (actor net, critic net) of tests/policy_mlp_reference.py, for the sizes."""
    lib = N.lib()
    sa, sc_ = specs(*nets)
    idx_t = None if idx is None else torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    need = int(lib.rdv_ppo_mlp_workspace_bytes(C.byref(sa), C.byref(sc_), max(n, 1)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if workspace is None else workspace
    ka, kc = int(lib.rdv_ppo_mlp_grad_floats(C.byref(sa), 1)), int(lib.rdv_ppo_mlp_grad_floats(C.byref(sc_), 0))
    ag, cg, sc = (torch.full((k,), float("nan"), device=DEV) for k in (ka, kc, N.PPO_SCALARS))
    lp, val = torch.full((max(n, 1),), float("nan"), device=DEV), torch.full((max(n, 1),), float("nan"), device=DEV)
    rows = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["old_log_prob"].data_ptr(), cols["advantages"].data_ptr(),
                     cols["returns"].data_ptr(), None if idx_t is None else idx_t.data_ptr(), cols["obs"].shape[0])
    out = N.PpoOut(ag.data_ptr(), cg.data_ptr(), sc.data_ptr(), lp.data_ptr(), val.data_ptr())
    rc = getattr(lib, fn)(pol._hip_handle(DEV) if actor is None else actor, pol._critic_handle(DEV) if critic is None else critic,
                          C.byref(rows), n, eps, ent, vf, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(out),
                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    if raw:
        return rc, lib.rdv_last_error().decode()
    N.check(rc)
    torch.cuda.synchronize()
    grads = []
    for flat, net, is_actor in ((ag.cpu().numpy().astype(np.float64), nets[0], True), (cg.cpu().numpy().astype(np.float64), nets[1], False)):
        at = 0
        for s in Q.shapes(net, is_actor):
            k = int(np.prod(s))
            grads.append(flat[at:at + k].reshape(s)); at += k
        assert at == flat.size
    return dict(grads=grads, scalars=dict(zip(P.SCALARS, sc.cpu().numpy().astype(np.float64))), log_prob=lp.cpu().numpy(), values=val.cpu().numpy(),
                raw=(ag, cg, sc, lp, val))


_MEMBERS = {}


def member(case):
    """(case dict, policy, device columns) of one entry of Q.CASES (as a tuple of tuples); made once, left unchanged."""
    if case not in _MEMBERS:
        pi, vf, act = case
        c = Q.make_case(pi, vf, act)
        _MEMBERS[case] = (c, make_policy(c["actor"], c["critic"]), device_columns(c))
    return _MEMBERS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_members():
    yield
    for _, pol, _ in _MEMBERS.values():
        pol.close()
    _MEMBERS.clear()


KEYS = [(tuple(pi), tuple(vf), act) for pi, vf, act in Q.CASES]
IDS = [Q.case_id(c) for c in Q.CASES]
FOUR_WAVES = [k for k in KEYS if k[0] == (64, 64, 64, 64)]
RELU_PAIR = ((32, 32), (64, 16), "relu")


def tensor_err(g, w):
    """max|g - w| / max|w|.  A reference tensor of zeros — a lone sample on the zero-gradient side of the clip has no actor gradient —
    leaves no relative error: it asks for zeros, by equality (0, or inf for any other entry)."""
    if not np.any(np.asarray(w)):
        return 0.0 if not np.any(np.asarray(g)) else float("inf")
    return P.rel_err(g, w)


def compare(names, got, ref, g32, s32):
    """rows (name, err, e32) of the accuracy rule: every gradient tensor and five scalars of one call against the fp64 reference, beside
    the float32 autograd yardstick."""
    rows = [(name, tensor_err(g, w), tensor_err(y, w)) for name, g, w, y in zip(names, got["grads"], ref["grads"], g32)]
    for name in P.SCALARS:
        if name != "clip_fraction":
            w = ref["scalars"][name]
            rows.append((name, abs(got["scalars"][name] - w) / abs(w), abs(s32[name] - w) / abs(w)))
    return rows


def measure(c, pol, cols, n, indexed):
    """One shape: the call, the fp64 reference, the float32 autograd yardstick -> rows (name, err, e32) and the pieces the test asserts on."""
    idx = P.index_vector(n) if indexed else None
    mb = P.take(c, idx if indexed else n)
    nets = (c["actor"], c["critic"])
    got = call(pol, nets, cols, n, idx)
    ref = Q.analytic64(*nets, *mb, eps=P.EPS, ent_coef=ENT, vf_coef=VF)
    g32, s32 = Q.autograd(*nets, *mb, eps=P.EPS, ent_coef=ENT, vf_coef=VF, dtype="float32")
    return compare(Q.names(*nets), got, ref, g32, s32), got, ref, mb


def assert_rule(label, rows, skip=()):
    """The accuracy rule on the rows of ``compare``: err <= C max(e32, 2^-23), C_GRAD for a gradient tensor, C_BOUND for a scalar."""
    worst = []
    for name, err, e32 in rows:
        bound = max(e32, FLOOR)
        print(f"{label} {name}: err {err:.3e} e32 {e32:.3e} ratio {err / bound:.3f}")
        if name not in skip and not err <= (C_GRAD if "." in name else C_BOUND) * bound:
            worst.append((name, err, e32))
    assert not worst, worst


def assert_clip_count(got, ref, n):
    count = got["scalars"]["clip_fraction"] * n                     # (the scalar is count / n rounded to float32)
    assert round(count) == round(ref["scalars"]["clip_fraction"] * n) and abs(count - round(count)) < 1e-3


def check_shape(c, pol, cols, label, n, indexed):
    rows, got, ref, mb = measure(c, pol, cols, n, indexed)
    obs = torch.from_numpy(np.array(mb[0])).to(DEV)
    # 1. values: the bits of policy.value on the gathered rows; log_prob: the means' fp32 budget through the density
    assert np.array_equal(got["values"], pol.value(obs).cpu().numpy())
    lp_err, lp_tol = np.abs(got["log_prob"].astype(np.float64) - ref["log_prob"]), Q.log_prob_budget(c["actor"], mb[0], mb[1])
    print(f"{label} n={n} indexed={indexed}: log_prob err/budget max {float((lp_err / lp_tol).max()):.3f}")
    assert (lp_err <= lp_tol).all(), float((lp_err / lp_tol).max())
    # 2. the gradients and 3. five scalars: err <= C max(e32, 2^-23); clip_fraction n: the reference's count exactly
    assert_rule(f"{label} n={n} indexed={indexed}", rows)
    assert_clip_count(got, ref, n)


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "indexed"])
@pytest.mark.parametrize("n", Q.SHAPES)
@pytest.mark.parametrize("case", KEYS, ids=IDS)
def test_loss_and_gradients_match_the_fp64_reference(case, n, indexed):
    c, pol, cols = member(case)
    check_shape(c, pol, cols, Q.case_id(case), n, indexed)


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "indexed"])
@pytest.mark.parametrize("n", Q.SMALL_GROUP_SHAPES)
@pytest.mark.parametrize("case", FOUR_WAVES, ids=[Q.case_id(c) for c in FOUR_WAVES])
def test_the_edge_of_a_four_wave_workgroup(case, n, indexed):
    """4 x 64: the parameter block leaves the CU's LDS room for four waves, a workgroup owns 128 rows (csrc/rdv_ppo_mlp.h): its edge."""
    c, pol, cols = member(case)
    check_shape(c, pol, cols, Q.case_id(case), n, indexed)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def buffer_of(cols):
    return dict(obs=cols["obs"], actions=cols["actions"], log_prob=cols["old_log_prob"], advantages=cols["advantages"], returns=cols["returns"])


# ---------------------------------------------------------------------------------------------------------- once each
@pytest.mark.parametrize("case", [RELU_PAIR, ((64, 64, 64, 64), (64, 64, 64, 64), "tanh")], ids=["32x32-64x16-relu", "4x64-tanh"])
def test_two_eager_calls_and_a_graph_replay_give_the_same_bits(case):
    c, pol, cols = member(case)
    buf = buffer_of(cols)
    idx = torch.as_tensor(P.index_vector(549), device=DEV)
    outs = []
    for _ in range(2):
        s = pol.ppo_grad(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
        outs.append([p.grad.clone() for p in pol.parameters()] + [torch.stack([s[k] for k in P.SCALARS])])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        pol.ppo_grad(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, check=False)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            s = pol.ppo_grad(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, check=False)
            sc = torch.stack([s[k] for k in P.SCALARS])
        for p in pol.parameters():
            p.grad.zero_()
        g.replay()
        stream.synchronize()
    outs.append([p.grad.clone() for p in pol.parameters()] + [sc])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert all(bool(torch.isfinite(a).all()) and bool((a != 0).any()) for a in outs[0][:-1])


def test_update_weights_then_ppo_grad_differentiates_the_new_weights():
    c, _, cols = member(RELU_PAIR)
    other = Q.nets([32, 32], [64, 16], "relu", seed=9)
    pol = make_policy(c["actor"], c["critic"])
    try:
        buf = buffer_of(cols)
        idx = torch.as_tensor(P.index_vector(257), device=DEV)
        pol.ppo_grad(buf, idx, clip_range=P.EPS)                                   # the handles exist and hold the old weights
        pol.update_weights(M.weights_dict(*other))
        s = pol.ppo_grad(buf, idx, clip_range=P.EPS)
        got = [p.grad.clone() for p in pol.parameters()]
        fresh = make_policy(*other)
        s_f = fresh.ppo_grad(buf, idx, clip_range=P.EPS)
        for a, p in zip(got, fresh.parameters()):
            assert torch.equal(a, p.grad)
        assert all(torch.equal(s[k], s_f[k]) for k in s)
        fresh.close()
    finally:
        pol.close()


@pytest.mark.parametrize("column", P.COLUMNS)
def test_a_nan_in_one_row_reaches_the_gradients_and_the_scalars(column):
    """The NaN rule of include/rdv.h, one column at a time, on pi = [32, 32], vf = [64, 16] ReLU: n = 549, one NaN in row 540.  Which
    tensors are NaN throughout and which scalars are NaN is the fp64 reference's pattern (``ppo_mlp_reference.nan_rule``: all actor
    tensors, all critic tensors); everything else is finite; a net whose inputs are clean keeps the bits of the clean call, and so do
    log_prob and values of every other row."""
    base, pol, cols = member(RELU_PAIR)
    nets = (base["actor"], base["critic"])
    n, row = 549, P.NAN_ROW
    c = P.with_nan(base, column, row)
    clean = call(pol, nets, cols, n)
    got = call(pol, nets, device_columns(c), n)
    with np.errstate(invalid="ignore"):
        ref = Q.analytic64(*nets, *P.take(c, n), eps=P.EPS, ent_coef=ENT, vf_coef=VF)
    rule = Q.nan_rule(*nets)[column]
    want = (tuple(rule[0]), tuple(rule[1]))
    assert Q.nan_pattern(*nets, ref["grads"], ref["scalars"]) == want
    assert Q.nan_pattern(*nets, got["grads"], got["scalars"]) == want
    a_names, c_names = Q.actor_names(*nets)
    for net, names in ((0, a_names), (1, c_names)):
        if not set(names) & set(want[0]):
            assert torch.equal(got["raw"][net].view(torch.int32), clean["raw"][net].view(torch.int32)), names
    others = np.arange(n) != row
    for key in ("log_prob", "values"):
        assert np.array_equal(bits(got[key][others]), bits(clean[key][others])), key
        assert bool(np.isnan(got[key][row])) == bool(np.isnan(ref[key][row])), key
    assert all(np.isfinite(got["scalars"][q]) for q in P.SCALARS if q not in want[1])


@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "indexed"])
def test_the_backward_pass_differentiates_the_clamped_observations(indexed):
    """[32, 16] ReLU by the recipe of ``ppo_reference.clamp_nets``: every eighth row has obs[3] in {62.9, 63, 64, 1e4, -64, -1e4}, read
    through weights of 2^-7 their size; dW1 is the product with the CLAMPED rows (tests/test_ppo_mlp_grad.py: the rule tells a product with
    the rows as given)."""
    c = Q.clamp_case()
    pol = make_policy(c["actor"], c["critic"])
    try:
        check_shape(c, pol, device_columns(c), "clamp 32x16-relu", 549, indexed)
    finally:
        pol.close()


def test_rows_at_the_relu_cap_contribute_nothing_through_the_capped_unit():
    """``ppo_mlp_reference.relu_clamp_case``: unit 0 of both first layers reaches 62.9, 63, 64 and 1e4.  The derivative is 1 at 62.9 and 0
    at 64 and 1e4 (the kernel's cap acted); the row at 63, whose class a last bit decides, carries no weight (advantage 0, return = the
    device's own value).  The rule holds against the fp64 reference; the CPU test shows it telling an uncapped derivative."""
    c, at = Q.relu_clamp_case()
    nets = (c["actor"], c["critic"])
    pol = make_policy(*nets)
    try:
        n = c["obs"].shape[0]
        first = call(pol, nets, device_columns(c), n)
        ret = np.array(c["returns"]); ret[at[1]] = first["values"][at[1]]
        c = P.with_columns(c, returns=ret)
        got = call(pol, nets, device_columns(c), n)
        mb = P.take(c, n)
        ref = Q.analytic64(*nets, *mb, eps=P.EPS, ent_coef=ENT, vf_coef=VF)
        hidden = ref["hidden"][0][0][at, 0]
        assert hidden[0] < 63.0 and np.all(hidden[2:] == 63.0)
        g32, s32 = Q.autograd(*nets, *mb, eps=P.EPS, ent_coef=ENT, vf_coef=VF, dtype="float32")
        assert np.array_equal(got["values"], pol.value(torch.from_numpy(np.array(mb[0])).to(DEV)).cpu().numpy())
        assert_rule("relu cap", compare(Q.names(*nets), got, ref, g32, s32))
    finally:
        pol.close()


def test_default_spec_handles_get_the_bits_of_rdv_ppo_loss_grad():
    c = P.make_case("random")
    nets = (c["actor"], c["critic"])
    pol = make_policy(*nets)
    try:
        cols = device_columns(c)
        idx = P.index_vector(549)
        a = call(pol, nets, cols, 549, idx)
        b = call(pol, nets, cols, 549, idx, fn="rdv_ppo_loss_grad")
        for x, y in zip(a["raw"], b["raw"]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        lib, (sa, sc) = N.lib(), specs(*nets)
        for n in (1, 256, 257, 65536):
            assert lib.rdv_ppo_mlp_workspace_bytes(C.byref(sa), C.byref(sc), n) >= lib.rdv_ppo_workspace_bytes(n)
    finally:
        pol.close()


def test_refusals_leave_the_handles_usable():
    c, pol, cols = member(RELU_PAIR)
    nets = (c["actor"], c["critic"])
    before = call(pol, nets, cols, 33)
    a, cr = pol._hip_handle(DEV), pol._critic_handle(DEV)
    small = torch.empty(64, dtype=torch.uint8, device=DEV)
    shipped = MlpPolicy(M.weights_dict(*P.random_nets())).to(DEV)
    pset = PolicySet([pol, pol], [256, 256])
    lstm = LstmPolicy(lstm_hidden_size=32, net_arch=[64, 64], n_rows=64)
    for kwargs, word in ((dict(actor=cr, critic=a), "swapped"), (dict(workspace=small), "workspace_bytes"), (dict(eps=0.0), "clip_range"),
                         (dict(ent=-1.0), "ent_coef"), (dict(vf=float("nan")), "vf_coef"), (dict(actor=shipped._hip_handle(DEV)), "mixed pair"),
                         (dict(critic=shipped._critic_handle(DEV)), "mixed pair"),
                         (dict(actor=pset._hip_handle(DEV)), "policy set"), (dict(critic=pset._critic_handle(DEV)), "policy set"),
                         (dict(actor=lstm._hip_handle(DEV)), "recurrent")):
        rc, msg = call(pol, nets, cols, 33, raw=True, **kwargs)
        assert rc == -1 and word in msg, (kwargs, msg)
    rc, msg = call(pol, nets, cols, 0, raw=True, workspace=small)
    assert rc == -1 and "n must be positive" in msg
    after = call(pol, nets, cols, 33)
    for x, y in zip(before["raw"], after["raw"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # the Python layer routes the pair the library refuses to autograd
    mixed = MlpPolicy(M.weights_dict(P.random_nets()[0], M.critic_of(M.dense([32, 32], "tanh")))).to(DEV)
    from reinforcement_learning_rendezvous_amd.ppo import hip_route
    assert hip_route(mixed) is None and hip_route(pol) == "mlp" and hip_route(shipped) == "shipped"
    s = mixed.ppo_grad(buffer_of(cols), torch.as_tensor(P.index_vector(33), device=DEV), clip_range=P.EPS)
    assert all(bool(torch.isfinite(v)) for v in s.values())
    shipped.close(); pset.close(); lstm.close(); mixed.close()


def test_ppo_grad_fills_grad_with_the_bits_of_the_c_call():
    c, pol, cols = member(RELU_PAIR)
    nets = (c["actor"], c["critic"])
    idx = P.index_vector(257)
    s = pol.ppo_grad(buffer_of(cols), torch.as_tensor(idx, device=DEV), clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=False)
    got = [p.grad.clone() for p in [t for lin in pol._layers("l") for t in (lin.weight, lin.bias)] + [pol.log_std]
           + [t for lin in pol._layers("v") for t in (lin.weight, lin.bias)]]
    direct = call(pol, nets, cols, 257, idx)
    for name, g, w in zip(Q.names(*nets), got, direct["grads"]):
        assert np.array_equal(bits(g.cpu().numpy()), bits(w)), name
    for k, name in enumerate(P.SCALARS):
        assert bits(float(s[name])) == bits(direct["raw"][2][k].item()), name


def test_normalised_advantages_match_the_fallback():
    """normalize_advantage=True: the HIP path against the autograd fallback of the same policy on the same minibatch, duplicates included:
    a check of the plumbing, to the tolerance of tests/test_gpu_ppo_grad.py (1e-4)."""
    c, pol, cols = member(RELU_PAIR)
    buf = buffer_of(cols)
    idx = torch.as_tensor(P.index_vector(257), device=DEV)
    s = pol.ppo_grad(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
    got = [p.grad.clone() for p in pol.parameters()]
    ref_pol = make_policy(c["actor"], c["critic"])
    ref_pol.backend = "torch"
    s_ref = ref_pol.ppo_grad(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
    for (name, _), g, p in zip(pol.named_parameters(), got, ref_pol.parameters()):
        assert P.rel_err(g.cpu().numpy(), p.grad.cpu().numpy()) < 1e-4, name
    for k in s:
        assert float(s[k]) == pytest.approx(float(s_ref[k]), rel=1e-4, abs=1e-6), k
    ref_pol.close()


def test_three_adam_steps_end_to_end():
    """[32, 32] ReLU (the reference's custom_networks.py): ppo_grad, clip_grad_norm_, Adam, update_weights, three times; afterwards the
    handles act as a fresh policy built from the modules' parameters, and the weights have moved."""
    c = Q.make_case([32, 32], [32, 32], "relu")
    pol = make_policy(c["actor"], c["critic"])
    start = make_policy(c["actor"], c["critic"])
    try:
        buf = buffer_of(device_columns(c))
        opt = torch.optim.Adam(pol.parameters(), lr=3e-4)
        gen = torch.Generator(device=DEV).manual_seed(2)
        from reinforcement_learning_rendezvous_amd.ppo import ppo_minibatches
        for idx in ppo_minibatches(P.ROWS, 400, gen):
            stats = pol.ppo_grad(buf, idx, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
            for name, p in pol.named_parameters():
                assert bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
            torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
            opt.step()
            pol.update_weights()
        assert all(bool(torch.isfinite(v)) for v in stats.values())
        layers = lambda prefix: pol._layers(prefix)
        actor = M.make_net([l.weight.detach().cpu().numpy() for l in layers("l")], [l.bias.detach().cpu().numpy() for l in layers("l")], "relu",
                           pol.log_std.detach().cpu().numpy())
        critic = M.make_net([l.weight.detach().cpu().numpy() for l in layers("v")], [l.bias.detach().cpu().numpy() for l in layers("v")], "relu")
        fresh = make_policy(actor, critic)
        obs = buf["obs"][:300]
        assert torch.equal(pol.act(obs, deterministic=True), fresh.act(obs, deterministic=True))
        assert torch.equal(pol.value(obs), fresh.value(obs))
        assert not torch.equal(pol.act(obs, deterministic=True), start.act(obs, deterministic=True))
        fresh.close()
    finally:
        pol.close(); start.close()

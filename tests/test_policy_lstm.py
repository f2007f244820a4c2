"""
CPU tests of the recurrent policy: tests/policy_lstm_reference.py pinned against torch.nn.LSTM in float64, the error budget and its power
to tell wrong restatements apart, the one-step budget (its tolerance against what it guards, its defects, the state corners and the
clamp on h, the classes' shifts), the routing probes' coverage, the host-only spec checks and refusals of include/rdv.h ("The recurrent
policy"), LstmPolicy's state-dict inference and its PyTorch fallback.  tests/test_gpu_policy_lstm.py holds the kernels to the same
reference.
"""
import ctypes as C
import functools
import io
import json
import zipfile

import numpy as np
import pytest

import advantages_reference as AR
import policy_lstm_reference as L
import policy_reference as R

torch = pytest.importorskip("torch")

from reinforcement_learning_rendezvous_amd import _native as N                   # noqa: E402
from reinforcement_learning_rendezvous_amd import LstmPolicy, PolicySet           # noqa: E402


def _policy(net, critic=None, **kw):
    return LstmPolicy(L.weights_dict(net, L.critic_of(net) if critic is None else critic), activation_fn=net["act"], **kw)


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_reference_equals_torch_lstm_in_float64(H):
    """8 steps with episode starts: NumPy float64 restatement against torch.nn.LSTM(17, H).double() + Linear layers, to 1e-12."""
    net = L.hot(H)
    T, n = 8, 40
    obs, starts = L.obs_sequence(n, T), L.episode_starts(n, T)
    out, hs, cs = L.run(net, obs, starts)
    lstm = torch.nn.LSTM(IN := 17, H).double()
    lins = [torch.nn.Linear(w.shape[1], w.shape[0]).double() for w in net["w"]]
    with torch.no_grad():
        for k, a in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(lstm, k).copy_(torch.from_numpy(net[a].astype(np.float64)))
        for lin, w, b in zip(lins, net["w"], net["b"]):
            lin.weight.copy_(torch.from_numpy(w.astype(np.float64))); lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        h = c = torch.zeros(1, n, H, dtype=torch.float64)
        for t in range(T):
            keep = torch.from_numpy(1.0 - starts[t].astype(np.float64))[None, :, None]
            y, (h, c) = lstm(torch.from_numpy(obs[t].astype(np.float64))[None], (h * keep, c * keep))
            x = y[0]
            for lin in lins[:-1]:
                x = torch.tanh(lin(x))
            x = lins[-1](x)
            assert np.abs(h[0].numpy() - hs[t]).max() < 1e-12 and np.abs(c[0].numpy() - cs[t]).max() < 1e-12
            assert np.abs(x.numpy() - out[t]).max() < 1e-12


@pytest.mark.parametrize("cid", list(L.CLASSES))
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_budget_tells_the_wrong_restatements_apart(H, cid):
    """Gate order i, f, o, g; state not zeroed at an episode start; b_hh dropped; c replaced by h: each leaves 1.5 e32 + A by a factor
    of at least 10 on the committed inputs, and the float32 evaluation itself stays inside the budget."""
    net = L.CLASSES[cid](H)
    obs, starts = L.obs_sequence(257), L.episode_starts(257)
    bud = L.budget(net, obs, starts)
    assert np.isfinite(bud["A_out"]).all() and (bud["A_out"] > 0).all() and (np.abs(bud["out64"]) < 0.999).all()   # the clip plays no part
    assert (bud["A_h"][0].max() < 2e-6) and (bud["A_out"][0].max() < 1e-4)          # step 0: no recurrence yet, the budget is the activations'
    for d in L.DEFECTS:
        f = L.defect_factor(net, obs, starts, d, bud)
        assert f >= 10.0, (H, cid, d, f)


# ------------------------------------------------------------------------------------- the one-step budget and the new classes
LOCAL_ROWS = 65


@functools.lru_cache(maxsize=None)
def _far_state(cid, H):
    """(net, obs of step 48, (h, c) a float32 run reaches after 48 steps, the one-step budget from there): computed once per class and H."""
    net = L.ALL_CLASSES[cid](H)
    obs, h, c = L.far_state(net, LOCAL_ROWS)
    return net, obs, h, c, L.local_budget(net, obs, None, h, c)


@pytest.mark.parametrize("cid", list(L.ALL_CLASSES))
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_classes_have_the_shifts_they_are_built_for(H, cid):
    net = L.ALL_CLASSES[cid](H)
    assert (R.documented_shift(net["w_ih"]), R.documented_shift(net["w_hh"])) == L.CLASS_SHIFTS[cid]
    assert L.cell_shift(net) == min(L.CLASS_SHIFTS[cid]) and L.cell_shift(net, "shift_is_max") == max(L.CLASS_SHIFTS[cid])
    base = L.hot(H)
    for k in ("w", "b"):                                                 # the change is to the cell only
        assert all(np.array_equal(x, y) for x, y in zip(net[k], base[k]))


def test_quantised_is_the_documented_two_term_split():
    """hi + lo carries w 2^s to 22 bits where both terms are normal; under a low shift the lo term goes subnormal and loses bits; a
    scaled weight of 65520 or more has no float16."""
    w = np.asarray([0.3751234, -0.0123457, 3000.0, 1e-5, 0.0, -59.99], np.float32)
    q10 = L.quantised(w[[0, 1, 3, 4]], 10)
    w10 = w[[0, 1, 3, 4]].astype(np.float64)
    assert (np.abs(q10 - w10) <= np.maximum(2.0 ** -22 * np.abs(w10), 2.0 ** -25 * 2.0 ** -10)).all() and q10[3] == 0.0
    assert L.quantised(w[[2, 5]], 3)[0] == 3000.0 and abs(L.quantised(w[[5]], 9)[0] - float(w[5])) <= 2.0 ** -22 * 60
    r3, r10 = (np.abs(L.quantised(w[:2], s) - w[:2].astype(np.float64)) for s in (3, 10))
    assert (r3 <= 2.0 ** -25).all() and r3[1] > 8 * r10[1] >= 0                     # -0.0123 x 2^3: its lo term is on the subnormal grid 2^-24
    assert (np.abs(L.quantised(w[:2], 10, lo_term=False) - w[:2]) > 100 * r10).all()
    assert not np.isfinite(L.quantised(w[[2]], 10)).any()


@pytest.mark.parametrize("cid", list(L.ALL_CLASSES))
@pytest.mark.parametrize("H", (32, 256))
def test_local_tolerance_is_a_hundredth_of_what_it_guards(H, cid):
    """48 steps from zero, then one: the one-step tolerance on the means is at most 1 % of the spread of the reference's means over the
    rows of that step (the condition that keeps the local check from asserting nothing), the means are inside the clip, the float32
    step is inside its own budget, and the state is where the class is meant to take it."""
    net, obs, h0, c0, bud = _far_state(cid, H)
    tol = {w: L.local_tolerance(bud, w) for w in ("out", "h", "c")}
    spread = float((bud["out64"].max(axis=0) - bud["out64"].min(axis=0)).min())
    print(f"TABLE H {H:3d} {cid:12s} tol out {tol['out']:.3g} h {tol['h']:.3g} c {tol['c']:.3g}  spread {spread:.3g}  tol/spread {tol['out'] / spread:.2g}  max|c| {np.abs(c0).max():.3g}")
    assert 0 < tol["out"] <= 0.01 * spread, (tol, spread)
    assert (np.abs(bud["out64"]) < 0.999).all() and np.isfinite(bud["A_out"]).all()
    assert tol["h"] < 2e-5 and (bud["e32_out"] <= bud["A_out"]).all()
    lo, hi = {"big_bias": (40.0, 48.0), "long_memory": (4.0, 12.0)}.get(cid, (0.0, 48.0))
    assert lo <= float(np.abs(c0).max()) <= hi
    if cid == "big_bias":                                                # gates at 0 and exactly 1 beside live ones
        parts = {}
        L.cell(net, R.clamp_obs(obs), h0, c0, np.zeros(len(obs), np.uint8), np.float32, parts=parts)
        g = np.concatenate([parts[k] for k in "ifo"], axis=1)
        assert (g < 1e-9).mean() > 0.05 and (g == 1).mean() > 0.05 and ((g > 0.05) & (g < 0.95)).mean() > 0.2    # (1 / (1 + e^30) is 9e-14)


@pytest.mark.parametrize("cid", list(L.ALL_CLASSES))
@pytest.mark.parametrize("H", (32, 256))
def test_local_budget_tells_the_wrong_restatements_apart(H, cid):
    """One step from the state after 48: every present defect (no_reset on a step where every third row starts), the cell's weights
    rounded to their hi term alone, and — where it moves a scaled outlier out of float16's range, 3000 x 2^10 — the larger shift for the
    smaller, each leave the one-step tolerance by a factor of at least 10 in one of the three comparisons the GPU tests make (outputs,
    h', c').  With outliers below 64 (hh_shift9) the larger shift still fits float16 (60 x 2^10 < 65504) and with equal shifts it is
    the same shift: no defect there."""
    net, obs, h0, c0, bud = _far_state(cid, H)
    some = (np.arange(LOCAL_ROWS) % 3 == 0).astype(np.uint8)
    found = {}
    for d in L.DEFECTS + L.QUANT_DEFECTS:
        if d == "shift_is_max" and min(L.CLASS_SHIFTS[cid]) > 3:
            continue
        found[d] = L.local_defect_factor(net, obs, some, h0, c0, d) if d == "no_reset" else L.local_defect_factor(net, obs, None, h0, c0, d, bud)
    print(f"TABLE H {H:3d} {cid:12s} " + "  ".join(f"{d} {f:.3g} ({w})" for d, (f, w) in found.items()))
    assert all(f >= 10.0 for f, _ in found.values()), found
    if cid in ("ih_shift3", "hh_shift3"):
        assert "shift_is_max" in found


def test_local_budget_from_zero_is_the_first_step_of_the_global_one():
    """The same reference values; the same budget plus the residual of the weights' quantisation, which at shift 10 adds little."""
    net = L.hot(64)
    obs, starts = L.obs_sequence(40, 1), L.episode_starts(40, 1)
    g, z = L.budget(net, obs, starts), np.zeros((40, 64), np.float32)
    loc = L.local_budget(net, obs[0], starts[0], z, z)
    for k in ("out64", "h64", "c64", "e32_out", "e32_h", "e32_c"):
        np.testing.assert_array_equal(loc[k], g[k][0])
    for k in ("A_out", "A_h", "A_c"):
        assert (loc[k] >= g[k][0]).all() and (loc[k] <= 1.25 * g[k][0]).all()


def test_state_corners_and_the_clamp():
    """|h| up to the clamp and past it, large |c|: the reference clamps h where it enters W_hh h and nowhere else (+-inf counts as +-63),
    a started row reads no state at all, and not clamping leaves the tolerance of every row beyond +-63 by a factor of at least 10."""
    net = L.hot(64)
    sc = L.state_corners(net)
    n = len(sc["obs"])
    bud = L.local_budget(net, sc["obs"], None, sc["h"], sc["c"])
    assert all(np.isfinite(bud[k]).all() for k in ("out64", "h64", "c64", "e32_out", "A_out", "A_h", "A_c"))
    kind = sc["kind"]
    clamped = L.local_budget(net, sc["obs"], None, np.clip(sc["h"], -63.0, 63.0), sc["c"])          # 64, 1e3 and inf all count as 63
    for k in ("out64", "h64", "c64"):
        np.testing.assert_array_equal(clamped[k], bud[k])
    ordinary = L.local_budget(net, sc["obs"], None, sc["h_ord"], sc["c_ord"])
    for r in sc["ordinary"]:
        np.testing.assert_array_equal(bud["out64"][r], ordinary["out64"][r])
    for r in range(n):
        f, what = L.local_defect_factor(net, sc["obs"], None, sc["h"], sc["c"], "h_not_clamped", bud, rows=[r])
        beyond = kind[r] in ("h=64", "h=-64", "h=1000", "h=-1000", "h=inf", "h=-inf")
        if beyond:
            print(f"TABLE h_not_clamped  row {r:2d} {kind[r]:8s} {f:.3g} ({what})")
        assert (f >= 10.0) if beyond else (f == 0.0), (r, kind[r], f)
    starts = np.ones(n, np.uint8)
    fresh = L.local_budget(net, sc["obs"], starts, sc["h"], sc["c"])
    zero = L.local_budget(net, sc["obs"], starts, np.zeros_like(sc["h"]), np.zeros_like(sc["c"]))
    np.testing.assert_array_equal(fresh["out64"], zero["out64"])


def test_the_recursion_matters_in_the_hot_class():
    """What the hot class is for: dropping W_hh h moves its outputs by far more than the default initialisation's."""
    obs, starts = L.obs_sequence(64), L.episode_starts(64)
    moved = {}
    for cid, make in L.CLASSES.items():
        net = make(256)
        cut = dict(net, w_hh=np.zeros_like(net["w_hh"]))
        moved[cid] = float(np.abs(L.run(net, obs, starts)[0] - L.run(cut, obs, starts)[0]).max())
    assert moved["hot"] > 3 * moved["default_init"] > 0, moved


@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_route_probes_cover_every_gate_fragment(H):
    assert L.route_coverage(H, L.ROUTE_PROBES) == 1.0
    net = L.route_probe(H, 0)
    assert ((net["w_hh"] != 0).sum(axis=1) == 1).all() and ((net["w_ih"] != 0).sum(axis=1) == 1).all()
    bud = L.budget(net, L.obs_sequence(33), L.episode_starts(33))
    assert (np.abs(bud["out64"]) < 0.999).all() and bud["A_out"].max() < 1e-3


# ---------------------------------------------------------------------------------------------------- spec checks, host-only
def _spec_rc(*a, **k):
    spec = N.LstmSpec.make(*a, **k)
    rc = N.lib().rdv_lstm_spec_check(C.byref(spec))
    return rc, N.lib().rdv_last_error().decode()


def test_spec_check_accepts_the_sweep_and_refuses_by_name():
    for H in L.HIDDEN_SIZES:
        for arch, act in (([64, 64], 0), ([16], 1), ([32, 32, 32], 2), ([64, 64, 64, 64], 0)):
            assert _spec_rc(H, arch, act)[0] == 0
    BAD_PARAMS, INVALID = -6, -1
    for kw, word in ((dict(hidden_size=48), "hidden_size = 48"), (dict(hidden_size=512), "hidden_size = 512"), (dict(n_layers=2), "n_layers = 2"),
                     (dict(n_layers=3), "n_layers = 3"), (dict(shared=1), "shared = 1")):
        args = dict(dict(hidden_size=256, trunk=[64, 64]), **kw)
        rc, msg = _spec_rc(**args)
        assert rc == BAD_PARAMS and word in msg, (kw, rc, msg)
    spec = N.LstmSpec.make(64, [64, 64]); spec.reserved = 1
    assert N.lib().rdv_lstm_spec_check(C.byref(spec)) == BAD_PARAMS and "reserved" in N.lib().rdv_last_error().decode()
    rc, msg = _spec_rc(64, [48])
    assert rc == INVALID and "hidden[0] = 48" in msg                     # the trunk is rdv_mlp_spec_check's
    assert N.lib().rdv_lstm_spec_check(None) == INVALID


def test_create_refuses_a_bad_spec_and_null_arrays_before_any_device():
    lib = N.lib()
    h = C.c_void_p()
    bad = N.LstmSpec.make(100, [64, 64])
    assert lib.rdv_lstm_policy_create(C.byref(bad), None, None, None, None, None, None, None, 8, 0, C.byref(h)) == -6
    assert lib.rdv_lstm_critic_create(C.byref(N.LstmSpec.make(64, [64, 64], n_layers=2)), None, None, None, None, None, None, 8, 0, C.byref(h)) == -6
    ok = N.LstmSpec.make(64, [64, 64])
    assert lib.rdv_lstm_policy_create(C.byref(ok), None, None, None, None, None, None, None, 8, 0, C.byref(h)) == -1
    assert lib.rdv_lstm_policy_create(C.byref(ok), None, None, None, None, None, None, None, 0, 0, C.byref(h)) == -1
    assert "n_rows" in lib.rdv_last_error().decode()
    for call in (lambda: lib.rdv_lstm_act(None, None, None, None, None, None, 8, 1, 0, 0, 0, None), lambda: lib.rdv_lstm_value(None, None, None, None, 8, 1, None),
                 lambda: lib.rdv_lstm_get_state(None, None, None, None), lambda: lib.rdv_lstm_set_state(None, None, None, None),
                 lambda: lib.rdv_lstm_reset_state(None, None, None), lambda: lib.rdv_lstm_set_weights(None, None, None, None, None, None, None, None, None)):
        assert call() == -5                                             # RDV_ERR_BAD_HANDLE
    assert lib.rdv_lstm_hidden_size(None) == -1


def test_python_refusals_by_name():
    for kw, word in ((dict(lstm_hidden_size=100), "lstm_hidden_size = 100"), (dict(n_lstm_layers=2), "n_lstm_layers = 2"),
                     (dict(shared_lstm=True), "shared_lstm"), (dict(enable_critic_lstm=False), "enable_critic_lstm")):
        with pytest.raises(ValueError, match=word):
            LstmPolicy(**kw)
    w = L.weights_dict(L.default_init(32), L.critic_of(L.default_init(32)))
    with pytest.raises(ValueError, match="lstm_critic"):
        LstmPolicy({k: v for k, v in w.items() if not k.startswith("lstm_critic.")})
    with pytest.raises(ValueError, match="more than one LSTM layer"):
        LstmPolicy(dict(w, **{"lstm_actor.weight_ih_l1": np.zeros((128, 32), np.float32)}))
    with pytest.raises(TypeError, match="not an MlpPolicy"):             # no recurrent members in policy sets
        PolicySet([LstmPolicy(lstm_hidden_size=32)], [8])


# ------------------------------------------------------------------------------------------------------ state-dict inference
@pytest.mark.parametrize("H,pi,vf,act", [(32, [64, 64], [64, 64], "tanh"), (128, [16], [32, 32, 32], "relu"), (256, [64, 64, 64, 64], [16, 16], "sigmoid")])
def test_architecture_is_inferred_from_the_shapes(H, pi, vf, act, tmp_path):
    actor, critic = L.default_init(H, pi, act), L.critic_of(L.default_init(H, vf, act, seed=7))
    w = L.weights_dict(actor, critic)
    pol = LstmPolicy(w, activation_fn=act)
    assert (pol.lstm_hidden_size, pol.pi_arch, pol.vf_arch, pol.activation) == (H, pi, vf, act)
    for k, v in pol.state_dict_sb3().items():
        np.testing.assert_array_equal(v, w[k], err_msg=k)
    np.savez(tmp_path / "w.npz", activation_fn=np.asarray(act), **w)
    again = LstmPolicy.from_npz(tmp_path / "w.npz")
    assert (again.lstm_hidden_size, again.pi_arch, again.vf_arch, again.activation) == (H, pi, vf, act)
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, buf)
    cls = {"tanh": "Tanh", "relu": "ReLU", "sigmoid": "Sigmoid"}[act]
    with zipfile.ZipFile(tmp_path / "m.zip", "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("data", json.dumps(dict(policy_kwargs=dict(activation_fn=f"<class 'torch.nn.modules.activation.{cls}'>", lstm_hidden_size=H))))
    z = LstmPolicy.from_sb3_zip(tmp_path / "m.zip")
    assert (z.lstm_hidden_size, z.pi_arch, z.vf_arch, z.activation) == (H, pi, vf, act)
    with pytest.raises(ValueError, match="does not fit"):
        LstmPolicy(dict(w, **{"lstm_critic.weight_ih_l0": np.zeros((4 * H, 16), np.float32)}))


# ------------------------------------------------------------------------------------------------------- the PyTorch fallback
def test_fallback_follows_the_reference_and_keeps_the_state_semantics():
    H, n, T = 64, 33, 6
    net, critic = L.hot(H), L.critic_of(L.hot(H, seed=9))
    pol = _policy(net, critic, backend="torch")
    obs, starts = L.obs_sequence(n, T), L.episode_starts(n, T)
    out64, h64, c64 = L.run(net, obs, starts)
    v64, vh64, _ = L.run(critic, obs, starts)
    for t in range(T):
        a = pol.act(torch.from_numpy(obs[t]), episode_start=starts[t])
        assert np.abs(a.numpy() - np.clip(out64[t], -1, 1)).max() < 2e-5
        h, c = pol.state
        assert np.abs(h.numpy() - h64[t]).max() < 2e-5 and np.abs(c.numpy() - c64[t]).max() < 2e-5
        before = [x.clone() for x in pol.critic_state] if t else None
        if t:
            peek = pol.value(torch.from_numpy(obs[t]), episode_start=starts[t], commit=False)
            assert all(torch.equal(x, y) for x, y in zip(before, pol.critic_state))           # commit = False writes nothing
        v = pol.value(torch.from_numpy(obs[t]), episode_start=starts[t])
        assert np.abs(v.numpy() - v64[t][:, 0]).max() < 2e-5
        if t:
            assert torch.equal(peek, v)
    # set_state(get_state()) is the identity; reset_state(mask) touches only the masked rows
    h, c = pol.state
    pol.state = (h, c)
    assert torch.equal(pol.state[0], h) and torch.equal(pol.state[1], c)
    mask = np.arange(n) % 4 == 1
    pol.reset_state(mask)
    h2, c2 = pol.state
    assert (h2[mask] == 0).all() and (c2[mask] == 0).all() and torch.equal(h2[~mask], h[~mask]) and torch.equal(c2[~mask], c[~mask])
    assert (pol.critic_state[0][mask] == 0).all()
    with pytest.raises(ValueError, match="rows"):
        pol.act(torch.zeros(5, 17))


def test_predict_has_sb3s_calling_convention():
    """save_new_trajectory.py:106-110: action, lstm_states = model.predict(obs, state=lstm_states, episode_start=..., deterministic=True)."""
    net = L.hot(32)
    pol, twin = _policy(net, backend="torch"), _policy(net, backend="torch")
    obs, starts = L.obs_sequence(1, 4), np.asarray([[1], [0], [0], [1]], np.uint8)
    state = None
    for t in range(4):
        action, state = pol.predict(obs[t][0], state=state, episode_start=starts[t], deterministic=True)
        want = twin.act(torch.from_numpy(obs[t]), episode_start=starts[t])
        assert action.shape == (6,) and state[0].shape == (1, 32) and state[1].shape == (1, 32)
        np.testing.assert_array_equal(action, want.numpy()[0])
    out64 = L.run(net, obs, starts)[0]
    assert np.abs(action - np.clip(out64[3][0], -1, 1)).max() < 2e-5


def test_fallback_advantages_are_the_critic_loop_plus_gae32():
    """LstmPolicy.advantages on CPU rows: T committing critic steps with the pending flags, then done[t-1]; one non-committing step on
    last_obs with done[T-1]; NumPy float32 GAE — against this test's own loop over a second policy; a second call goes on."""
    H, T, n = 32, 5, 12
    net, critic = L.default_init(H), L.critic_of(L.hot(H, seed=3))
    pol, twin = _policy(net, critic, backend="torch"), _policy(net, critic, backend="torch")
    rng = np.random.default_rng(5)
    for call in range(2):
        ro = dict(obs=torch.from_numpy(L.obs_sequence(n, T, seed=70 + call)), reward=torch.from_numpy(rng.normal(size=(T, n)).astype(np.float32)),
                  done=torch.from_numpy((rng.random((T, n)) < 0.3).astype(np.uint8)), last_obs=torch.from_numpy(R.distinct_rows(n, seed=90 + call)))
        got = pol.advantages(dict(ro), gamma=0.98, gae_lambda=0.9)
        flags = np.ones(n, np.uint8) if call == 0 else last_done
        values = np.zeros((T, n), np.float32)
        for t in range(T):
            values[t] = twin.value(ro["obs"][t], episode_start=flags).numpy()
            flags = ro["done"][t].numpy()
        last_value = twin.value(ro["last_obs"], episode_start=flags, commit=False).numpy()
        last_done = flags
        adv, ret = AR.gae32(ro["reward"].numpy(), ro["done"].numpy(), values, last_value, 0.98, 0.9)
        np.testing.assert_array_equal(got["values"].numpy(), values)
        np.testing.assert_array_equal(got["last_value"].numpy(), last_value)
        np.testing.assert_array_equal(got["advantages"].numpy(), adv)
        np.testing.assert_array_equal(got["returns"].numpy(), ret)
        for x, y in zip(pol.critic_state, twin.critic_state):
            assert torch.equal(x, y)


def test_state_at_start_on_the_torch_backend_follows_the_host_flags():
    """Two rollouts and an act on the PyTorch path: the flags are the host value ``_pending`` (True, False, or a copy of done[T-1]) and
    no device mirror exists.  Actor: what RendezvousBatch.rollout leaves through ``_set_pending``; critic: ``advantages`` itself.
    ``state_at_start`` is the state, zero on exactly the rows the last rollout ended on, and the whole state behind an act / a value."""
    H, T, n = 32, 4, 12
    net, critic = L.hot(H), L.critic_of(L.hot(H, seed=3))
    pol = _policy(net, critic, backend="torch", n_rows=n)
    rng = np.random.default_rng(6)
    obs = torch.from_numpy(L.obs_sequence(n, T + 1, seed=80))
    for call in range(2):
        done = torch.from_numpy((rng.random((T, n)) < 0.4).astype(np.uint8))
        assert 0 < int(done[T - 1].sum()) < n
        for t in range(T):                                                        # the act + step loop a rollout is defined by
            pol.act(obs[t], episode_start=pol._pending_flags("l", obs.device) if t == 0 else done[t - 1])
        pol._set_pending("l", done[T - 1], obs.device)
        pol.advantages(dict(obs=obs[:T], reward=torch.zeros(T, n), done=done, last_obs=obs[T]))
        last = done[T - 1].clone()
        done[T - 1] = 1 - done[T - 1]                                             # the flags are a copy: the caller's buffer may move on
        for prefix, state in (("l", pol.state), ("v", pol.critic_state)):
            assert isinstance(pol._pending[prefix], torch.Tensor) and torch.equal(pol._pending[prefix], last)
            assert torch.equal(pol._pending_flags(prefix, obs.device), last)
            h0, c0 = pol.state_at_start(prefix)
            keep = last == 0
            assert (h0[~keep] == 0).all() and (c0[~keep] == 0).all() and torch.equal(h0[keep], state[0][keep]) and torch.equal(c0[keep], state[1][keep])
            assert float(h0[keep].abs().min(dim=1).values.max()) > 0.0
    pol.act(obs[T])
    pol.value(obs[T], commit=False)
    assert pol._pending == {"l": False, "v": pol._pending["v"]} and isinstance(pol._pending["v"], torch.Tensor)    # a peek commits nothing
    pol.value(obs[T])
    assert pol._pending == {"l": False, "v": False} and pol._dev_pending == {}
    for prefix, state in (("l", pol.state), ("v", pol.critic_state)):
        for x, y in zip(pol.state_at_start(prefix), state):
            assert torch.equal(x, y)

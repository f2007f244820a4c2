"""
CPU tests of the learner-ready rollout columns (include/rdv.h: rdv_gae, rdv_rollout_advantages, rdv_policy_set_weights): the PyTorch
restatement of the GAE sequence against SB3's loop in NumPy float32 (tests/advantages_reference.py), that loop against its float64
form, the argument checks of the C ABI that need no GPU, and MlpPolicy.advantages / update_weights on the PyTorch modules.
"""
import ctypes as C

import numpy as np
import pytest

import advantages_reference as AR
import policy_mlp_reference as M
from helpers import shipped_policy
from reinforcement_learning_rendezvous_amd import _native as N

torch = pytest.importorskip("torch")

U32 = 2.0 ** -24          # unit roundoff of float32, round to nearest


def _tensors(case_inputs):
    return [torch.from_numpy(x) for x in case_inputs]


@pytest.mark.parametrize("case", AR.all_cases(), ids=AR.case_id)
def test_gae_on_cpu_tensors_equals_the_numpy_float32_loop(case):
    from reinforcement_learning_rendezvous_amd import gae
    T, n, pat, g, lam = case
    x = AR.inputs(T, n, pat)
    want_a, want_r = AR.gae32(*x, g, lam)
    adv, ret = gae(*_tensors(x), gamma=g, gae_lambda=lam)
    assert adv.dtype == torch.float32 and tuple(adv.shape) == (T, n)
    assert np.array_equal(adv.numpy(), want_a) and np.array_equal(ret.numpy(), want_r)
    # `out` is written in place and returned
    out = (torch.empty(T, n), torch.empty(T, n))
    got = gae(*_tensors(x), gamma=g, gae_lambda=lam, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], adv) and torch.equal(out[1], ret)


def test_gae_defaults_are_sb3s_and_a_nan_stays_in_its_env():
    from reinforcement_learning_rendezvous_amd import gae
    x = list(AR.inputs(33, 65, "bernoulli", seed=2))
    assert torch.equal(gae(*_tensors(x))[0], torch.from_numpy(AR.gae32(*x, 0.99, 0.95)[0]))
    x[0][20, 7] = np.nan
    adv, ret = gae(*_tensors(x))
    want_a, want_r = AR.gae32(*x, 0.99, 0.95)
    assert np.array_equal(adv.numpy(), want_a, equal_nan=True) and np.array_equal(ret.numpy(), want_r, equal_nan=True)
    bad = torch.isnan(adv) | torch.isnan(ret)
    assert bad[:, 7].any() and not bad[21:, 7].any() and not bad[:, [i for i in range(65) if i != 7]].any()


@pytest.mark.parametrize("case", AR.all_cases(), ids=AR.case_id)
def test_the_float32_loop_agrees_with_the_float64_loop(case):
    """Sanity of the helper.  With u = 2^-24, Mr = max|reward|, Mv = max|values, last_value|, and gamma, gamma * lambda <= 1:
    delta carries the rounding of (float)gamma and of g * nv (2 u Mv), of the sum with the reward (u (Mr + Mv)) and of the difference
    with values[t] (u (Mr + 2 Mv)): u D, D = 2 Mr + 5 Mv.  |A| <= T (Mr + 2 Mv) = Amax (a sum of at most T deltas).  One step of the
    chain adds the rounding of (float)(gamma lambda) and of the product with A (2 u Amax) and of the sum (u Amax) to the carried
    error, which c <= 1 does not grow: e_A <= T u (D + 3 Amax); returns add u (Amax + Mv).  Second-order terms and the float64 loop's own
    roundings are below 1e-4 of that: a factor 1.01."""
    T, n, pat, g, lam = case
    x = AR.inputs(T, n, pat)
    a32, r32 = AR.gae32(*x, g, lam)
    a64, r64 = AR.gae64(*x, g, lam)
    mr, mv = float(np.abs(x[0]).max()), float(max(np.abs(x[2]).max(), np.abs(x[3]).max()))
    amax = T * (mr + 2 * mv)
    bound_a = 1.01 * T * U32 * ((2 * mr + 5 * mv) + 3 * amax)
    bound_r = bound_a + 1.01 * U32 * (amax + mv)
    err_a, err_r = float(np.abs(a32 - a64).max()), float(np.abs(r32 - r64).max())
    print(f"{AR.case_id(case)}: |A32 - A64| = {err_a:.3e} (bound {bound_a:.3e}), returns {err_r:.3e} (bound {bound_r:.3e})")
    assert err_a <= bound_a and err_r <= bound_r
    assert float(np.abs(a64).max()) <= amax


# ----------------------------------------------------------------------------------------------------- C ABI, no GPU needed
FAKE = 0x1000      # a non-null "device pointer": the argument checks never dereference a data pointer


def _gae_call(**kw):
    a = dict(reward=FAKE, done=FAKE, values=FAKE, last_value=FAKE, n_steps=4, n=8, gamma=0.99, gae_lambda=0.95, advantages=FAKE, returns=FAKE)
    a.update(kw)
    rc = N.lib().rdv_gae(a["reward"], a["done"], a["values"], a["last_value"], a["n_steps"], a["n"], a["gamma"], a["gae_lambda"],
                         a["advantages"], a["returns"], 0, None)
    return rc, N.lib().rdv_last_error().decode()


@pytest.mark.parametrize("name", ["reward", "done", "values", "last_value", "advantages", "returns"])
def test_rdv_gae_refuses_a_null_pointer_by_name(name):
    rc, msg = _gae_call(**{name: None})
    assert rc == -1 and N.ERROR_NAMES[rc] == "RDV_ERR_INVALID_ARGUMENT" and "rdv_gae" in msg and name in msg


@pytest.mark.parametrize("kw,word", [(dict(n_steps=0), "n_steps"), (dict(n_steps=-3), "n_steps"), (dict(n=0), "n must"), (dict(n=-1), "n must"),
                                     (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=-0.1), "gamma"),
                                     (dict(gamma=float("inf")), "gamma"), (dict(gae_lambda=1.5), "gae_lambda"),
                                     (dict(gae_lambda=float("nan")), "gae_lambda"), (dict(gae_lambda=-0.1), "gae_lambda")])
def test_rdv_gae_refuses_sizes_and_discounts_by_name(kw, word):
    rc, msg = _gae_call(**kw)
    assert rc == -1 and word in msg, msg
    if "gamma" in kw:
        assert "gae_lambda" not in msg


def _rollout_advantages_call(critic=None, rows=None, out=None, n_steps=4, n=8, gamma=0.99, gae_lambda=0.95, rows_null=False, out_null=False):
    r = N.RolloutOut(FAKE, None, FAKE, FAKE, None, FAKE)        # actions and log_prob may be null here
    o = N.AdvantageOut(FAKE, FAKE, FAKE, FAKE)
    for k, v in (rows or {}).items():
        setattr(r, k, v)
    for k, v in (out or {}).items():
        setattr(o, k, v)
    rc = N.lib().rdv_rollout_advantages(critic, None if rows_null else C.byref(r), n_steps, n, gamma, gae_lambda,
                                        None if out_null else C.byref(o), None)
    return rc, N.lib().rdv_last_error().decode()


def test_rdv_rollout_advantages_argument_checks_without_a_gpu():
    for kw, word in [(dict(rows_null=True), "rows"), (dict(out_null=True), "out"), (dict(rows=dict(obs=None)), "rows->obs"),
                     (dict(rows=dict(reward=None)), "rows->reward"), (dict(rows=dict(done=None)), "rows->done"),
                     (dict(rows=dict(last_obs=None)), "rows->last_obs"), (dict(out=dict(values=None)), "out->values"),
                     (dict(out=dict(last_value=None)), "out->last_value"), (dict(out=dict(advantages=None)), "out->advantages"),
                     (dict(out=dict(returns=None)), "out->returns"), (dict(n_steps=0), "n_steps"), (dict(n=0), "n must"),
                     (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=-0.1), "gamma"),
                     (dict(gae_lambda=1.5), "gae_lambda"), (dict(gae_lambda=float("nan")), "gae_lambda"), (dict(gae_lambda=-0.1), "gae_lambda")]:
        rc, msg = _rollout_advantages_call(**kw)
        assert rc == -1 and "rdv_rollout_advantages" in msg and word in msg, (kw, rc, msg)
    rc, msg = _rollout_advantages_call()                          # everything else in order: the null critic handle
    assert rc == -5 and N.ERROR_NAMES[rc] == "RDV_ERR_BAD_HANDLE" and "rdv_policy" in msg


def test_rdv_policy_set_weights_refuses_a_null_handle():
    assert N.lib().rdv_policy_set_weights(None, None, None, None, None) == -5


# ------------------------------------------------------------------------------------------------------- MlpPolicy on the CPU
def _rollout_shaped(T, n, seed=5):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.uniform(-1, 1, size=s).astype(np.float32))
    return dict(obs=f(T, n, 17), actions=f(T, n, 6), reward=f(T, n) * 3, done=torch.from_numpy((rng.random((T, n)) < 0.1).astype(np.uint8)),
                log_prob=f(T, n), last_obs=f(n, 17))


@pytest.mark.parametrize("which", ["shipped", "relu32x32"])
def test_policy_advantages_on_cpu_rows_is_the_modules_values_plus_gae32(which):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    if which == "shipped":
        pol = shipped_policy()
        pol.backend = "torch"
    else:
        net = M.dense([32, 32], "relu")
        pol = MlpPolicy(M.weights_dict(net, M.critic_of(M.dense([32, 32], "relu", seed=22))), activation_fn="relu", backend="torch")
    assert pol.has_critic
    T, n = 9, 37
    ro = _rollout_shaped(T, n)
    got = pol.advantages(ro, gamma=0.98, gae_lambda=0.9)
    assert got is ro and set(ro) >= {"values", "last_value", "advantages", "returns", "actions", "log_prob"}
    values, last_value = pol.value(ro["obs"]), pol.value(ro["last_obs"])
    assert torch.equal(ro["values"], values) and torch.equal(ro["last_value"], last_value)
    want_a, want_r = AR.gae32(ro["reward"].numpy(), ro["done"].numpy(), values.numpy(), last_value.numpy(), 0.98, 0.9)
    assert np.array_equal(ro["advantages"].numpy(), want_a) and np.array_equal(ro["returns"].numpy(), want_r)
    # the four columns are allocated once: a second call writes the same tensors, through `ro` itself or through `out`
    ptrs = {k: ro[k].data_ptr() for k in ("values", "last_value", "advantages", "returns")}
    pol.advantages(ro, gamma=0.98, gae_lambda=0.9)
    fresh = _rollout_shaped(T, n, seed=6)
    pol.advantages(fresh, out=ro)
    assert all(ro[k].data_ptr() == p and fresh[k].data_ptr() == p for k, p in ptrs.items())
    with pytest.raises(ValueError, match="reward"):
        pol.advantages(dict(fresh, reward=fresh["reward"].double()))
    with pytest.raises(ValueError, match="gamma"):
        pol.advantages(fresh, gamma=1.5)


def test_policy_advantages_needs_a_critic():
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    with pytest.raises(ValueError, match="critic"):
        MlpPolicy(weights=None, backend="torch").advantages(_rollout_shaped(2, 3))


def test_gae_refuses_inputs_by_name():
    from reinforcement_learning_rendezvous_amd import gae
    r, d, v, lv = _tensors(AR.inputs(7, 64, "bernoulli"))
    with pytest.raises(ValueError, match="reward"):
        gae(r.double(), d, v, lv)
    with pytest.raises(ValueError, match="values"):
        gae(r, d, v.t().contiguous().t(), lv)              # transposed: right shape, not contiguous
    with pytest.raises(ValueError, match="done"):
        gae(r, d.to(torch.float32), v, lv)
    with pytest.raises(ValueError, match="last_value"):
        gae(r, d, v, lv[:-1])
    with pytest.raises(ValueError, match="gae_lambda"):
        gae(r, d, v, lv, gae_lambda=float("nan"))
    with pytest.raises(ValueError, match="returns"):
        gae(r, d, v, lv, out=(torch.empty(7, 64), torch.empty(64, 7)))


@pytest.mark.parametrize("arch,act", [([64, 64], "tanh"), ([16, 32], "sigmoid")])
def test_update_weights_on_a_cpu_policy_is_a_fresh_policy_of_the_dict(arch, act):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    mk = lambda seed: M.weights_dict(M.dense(arch, act, seed=seed), M.critic_of(M.dense(arch, act, seed=seed + 50)))
    pol = MlpPolicy(mk(1), activation_fn=act, backend="torch", seed=4)
    pol._calls = 7
    new = mk(2)
    fresh = MlpPolicy(new, activation_fn=act, backend="torch")
    obs = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, size=(50, 17)).astype(np.float32))
    assert not torch.equal(pol.mean(obs), fresh.mean(obs)) and not torch.equal(pol.value(obs), fresh.value(obs))
    pol.update_weights(new)
    assert torch.equal(pol.mean(obs), fresh.mean(obs)) and torch.equal(pol.value(obs), fresh.value(obs))
    assert torch.equal(pol.log_std, fresh.log_std)
    assert pol._calls == 7 and pol.noise_seed == 4
    pol.update_weights()                                            # nothing to push without a HIP handle: no error, no change
    assert torch.equal(pol.mean(obs), fresh.mean(obs))
    # a wrong shape raises and leaves the modules as they were
    bad = dict(new)
    bad["action_net.weight"] = np.zeros((6, arch[-1] + 1), np.float32)
    bad["mlp_extractor.policy_net.0.weight"] = np.zeros((arch[0], 17), np.float32)
    with pytest.raises(ValueError, match="action_net.weight"):
        pol.update_weights(bad)
    assert torch.equal(pol.mean(obs), fresh.mean(obs))

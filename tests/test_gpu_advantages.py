"""
GPU tests (run with `-m gpu`) of the learner-ready rollout columns: the GAE kernel (csrc/rdv_advantages.h, rdv_gae) against SB3's loop
in NumPy float32 (tests/advantages_reference.py) by EQUALITY — a kernel built with FMA contraction, or with gamma * lambda rounded
before the product, differs in the last bit and fails —, rdv_rollout_advantages on real rollouts, RendezvousBatch.collect against the
two calls it is made of, and rdv_policy_set_weights (MlpPolicy.update_weights) against freshly built policies.
"""
import numpy as np
import pytest

import advantages_reference as AR
import policy_mlp_reference as M
from helpers import gpu_batch, shipped_policy, to_numpy
from reinforcement_learning_rendezvous_amd.params import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cuda(xs):
    return [torch.from_numpy(x).to(DEV) for x in xs]


@pytest.mark.parametrize("case", AR.all_cases(), ids=AR.case_id)
def test_rdv_gae_equals_the_numpy_float32_loop(case):
    from reinforcement_learning_rendezvous_amd import gae
    T, n, pat, g, lam = case
    x = AR.inputs(T, n, pat)
    want_a, want_r = AR.gae32(*x, g, lam)
    adv, ret = gae(*_cuda(x), gamma=g, gae_lambda=lam)
    assert adv.is_cuda and adv.dtype == torch.float32 and tuple(adv.shape) == (T, n)
    assert torch.equal(adv.cpu(), torch.from_numpy(want_a)), "advantages"
    assert torch.equal(ret.cpu(), torch.from_numpy(want_r)), "returns"


def test_rdv_gae_keeps_a_nan_in_its_env():
    from reinforcement_learning_rendezvous_amd import gae
    T, n, env = 33, 65, 7
    x = list(AR.inputs(T, n, "bernoulli", seed=2))
    x[1][20:, env] = 0                           # no episode end between the NaN and the last step: it is carried to t = 0 ... 20
    x[1][:20, env] = 0
    x[0][20, env] = np.nan
    adv, ret = (to_numpy(t) for t in gae(*_cuda(x)))
    want_a, want_r = AR.gae32(*x, 0.99, 0.95)
    assert np.array_equal(adv, want_a, equal_nan=True) and np.array_equal(ret, want_r, equal_nan=True)
    bad = np.isnan(adv) | np.isnan(ret)
    others = [i for i in range(n) if i != env]
    assert bad[:21, env].all() and not bad[21:, env].any() and not bad[:, others].any()


def test_gae_refuses_inputs_by_name():
    from reinforcement_learning_rendezvous_amd import gae
    r, d, v, lv = _cuda(AR.inputs(7, 64, "bernoulli"))
    with pytest.raises(ValueError, match="reward"):
        gae(r.double(), d, v, lv)                                  # float64
    with pytest.raises(ValueError, match="values"):
        gae(r, d, v.t().contiguous().t(), lv)                      # transposed: the right shape, not contiguous
    with pytest.raises(ValueError, match="done"):
        gae(r, d.cpu(), v, lv)                                     # a CPU `done` beside CUDA rewards
    adv, _ = gae(r, d, v, lv)                                      # ... and the same tensors are accepted as they are
    assert torch.isfinite(adv).all()


def _general_policy():
    """[32, 32] ReLU actor and critic of policy_mlp_reference.dense."""
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    w = M.weights_dict(M.dense([32, 32], "relu"), M.critic_of(M.dense([32, 32], "relu", seed=22)))
    return MlpPolicy(w, activation_fn="relu", seed=3).to(DEV)


@pytest.mark.parametrize("which", ["shipped", "relu32x32"])
def test_rollout_advantages_on_a_real_rollout(which):
    T, n = 48, 1000
    env = gpu_batch(n, params=make_params(t_max=30.0), seed=9)          # time-outs, bubble exits and resets all occur within 48 steps
    pol = shipped_policy(DEV, noise_seed=3) if which == "shipped" else _general_policy()
    assert pol.has_critic and pol.shipped_arch == (which == "shipped")
    env.reset()
    ro = env.rollout(pol, T)
    assert int(ro["done"].sum()) > 0
    rows = {k: v.clone() for k, v in ro.items()}
    got = pol.advantages(ro, gamma=0.99, gae_lambda=0.95)
    assert got is ro and all(torch.equal(ro[k], v) for k, v in rows.items())      # the rollout's rows are only read
    values, last_value = pol.value(ro["obs"]), pol.value(ro["last_obs"])
    assert tuple(values.shape) == (T, n) and torch.equal(ro["values"], values), "values vs rdv_policy_value"
    assert torch.equal(ro["last_value"], last_value), "last_value vs rdv_policy_value"
    want_a, want_r = AR.gae32(to_numpy(ro["reward"]), to_numpy(ro["done"]), to_numpy(values), to_numpy(last_value), 0.99, 0.95)
    assert torch.equal(ro["advantages"].cpu(), torch.from_numpy(want_a)), "advantages vs gae32"
    assert torch.equal(ro["returns"].cpu(), torch.from_numpy(want_r)), "returns vs gae32"
    # an actor handle is refused in rdv_policy_value's words
    from reinforcement_learning_rendezvous_amd import _native as N
    import ctypes as C
    r = N.RolloutOut(ro["obs"].data_ptr(), None, ro["reward"].data_ptr(), ro["done"].data_ptr(), None, ro["last_obs"].data_ptr())
    o = N.AdvantageOut(*[ro[f].data_ptr() for f, _ in N.AdvantageOut._fields_])
    assert N.lib().rdv_rollout_advantages(pol._hip_handle(torch.device(DEV)), C.byref(r), T, n, 0.99, 0.95, C.byref(o), None) == -1
    assert b"this handle is an actor" in N.lib().rdv_last_error()
    env.close(); pol.close()


def test_collect_is_rollout_followed_by_advantages():
    T, n = 16, 777
    p = make_params(t_max=30.0)
    one, two = gpu_batch(n, params=p, seed=9), gpu_batch(n, params=p, seed=9)
    p1, p2 = shipped_policy(DEV, noise_seed=3), shipped_policy(DEV, noise_seed=3)
    one.reset(); two.reset()
    got = one.collect(p1, T, gamma=0.97, gae_lambda=0.9)
    want = p2.advantages(two.rollout(p2, T), gamma=0.97, gae_lambda=0.9)
    assert p1._calls == T == p2._calls
    assert set(got) == set(want) == {"obs", "actions", "reward", "done", "log_prob", "last_obs", "values", "last_value", "advantages", "returns"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(one.obs, two.obs) and torch.equal(one.get_state(), two.get_state())
    # the dict passed back as `out`: every buffer is reused, and the rows are those of the second pair of calls
    ptrs = {k: v.data_ptr() for k, v in got.items()}
    again = one.collect(p1, T, gamma=0.97, gae_lambda=0.9, out=got)
    want2 = p2.advantages(two.rollout(p2, T), gamma=0.97, gae_lambda=0.9)
    assert p1._calls == 2 * T
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    for k in want2:
        assert torch.equal(again[k], want2[k]), k
    assert not torch.equal(want2["obs"], want["obs"])
    for x in (one, two, p1, p2):
        x.close()


def _perturbed(pol, seed):
    """Every parameter of `pol`'s modules moved (in place), and the SB3-keyed dict of the result."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in pol.parameters():
            prm.add_((torch.randn(prm.shape, generator=g) * 0.05).to(prm.device))
    out = {"log_std": to_numpy(pol.log_std).copy()}
    for trunk, head, prefix in (("policy_net", "action_net", "l"), ("value_net", "value_net", "v")):
        layers = pol._layers(prefix)
        for l, lin in enumerate(layers[:-1]):
            out[f"mlp_extractor.{trunk}.{2 * l}.weight"], out[f"mlp_extractor.{trunk}.{2 * l}.bias"] = to_numpy(lin.weight).copy(), to_numpy(lin.bias).copy()
        out[f"{head}.weight"], out[f"{head}.bias"] = to_numpy(layers[-1].weight).copy(), to_numpy(layers[-1].bias).copy()
    return out


def _make_policy(which, seed=3):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    if which == "shipped":
        return shipped_policy(DEV, noise_seed=seed)
    w = M.weights_dict(M.dense([16, 32], "sigmoid"), M.critic_of(M.dense([16, 32], "sigmoid", seed=22)))
    return MlpPolicy(w, activation_fn="sigmoid", seed=seed).to(DEV)


def _outputs(pol, obs):
    """act (stochastic, deterministic), value and an 8-step rollout of a batch of its own, from call counter 0."""
    pol._calls = 0
    env = gpu_batch(obs.shape[0], seed=5)
    env.reset()
    out = dict(sample=pol.act(obs, deterministic=False).clone(), mean=pol.act(obs, deterministic=True).clone(), value=pol.value(obs).clone())
    out.update({"ro_" + k: v.clone() for k, v in env.rollout(pol, 8).items()})
    env.close()
    return out


@pytest.mark.parametrize("which", ["shipped", "sigmoid16x32"])
def test_update_weights_equals_a_fresh_policy_of_the_new_weights(which):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    n = 1000
    obs = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, size=(n, 17)).astype(np.float32)).to(DEV)
    pol = _make_policy(which)
    before = _outputs(pol, obs)                                   # creates the actor and the critic handle
    handles = (pol._hip[0].value, pol._hip_critic[0].value)
    new = _perturbed(pol, seed=8)
    calls, key = pol._calls, pol.noise_seed
    pol.update_weights()                                               # the modules' current parameters
    assert (pol._hip[0].value, pol._hip_critic[0].value) == handles and (pol._calls, pol.noise_seed) == (calls, key)
    after = _outputs(pol, obs)
    fresh = MlpPolicy(new, activation_fn=pol.activation, seed=pol.noise_seed).to(DEV)
    want = _outputs(fresh, obs)
    for k in want:
        assert torch.equal(after[k], want[k]), k
    assert not torch.equal(after["mean"], before["mean"]) and not torch.equal(after["value"], before["value"])
    # ... and with a dict: back to where a third policy stands
    other = _make_policy(which)
    back = _perturbed(other, seed=9)
    pol.update_weights(back)
    got, want = _outputs(pol, obs), _outputs(other, obs)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for x in (pol, fresh, other):
        x.close()


def test_update_weights_refuses_a_non_finite_weight_and_keeps_the_block():
    from reinforcement_learning_rendezvous_amd._native import RdvError
    obs = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, size=(300, 17)).astype(np.float32)).to(DEV)
    pol = _make_policy("shipped")
    mean, value = pol.act(obs, deterministic=True).clone(), pol.value(obs).clone()
    kept = float(pol.l2.weight[3, 5])
    with torch.no_grad():
        pol.l2.weight[3, 5] = float("inf")
        pol.v1.weight[0, 0] = float("nan")
    with pytest.raises(RdvError, match="RDV_ERR_BAD_PARAMS"):
        pol.update_weights()
    assert torch.equal(pol.act(obs, deterministic=True), mean)
    with torch.no_grad():
        pol.l2.weight[3, 5] = kept
    with pytest.raises(RdvError, match="RDV_ERR_BAD_PARAMS"):         # the actor's block is fine now, the critic's is not
        pol.update_weights()
    assert torch.equal(pol.value(obs), value) and torch.equal(pol.act(obs, deterministic=True), mean)
    pol.close()


def test_update_weights_is_ordered_on_the_callers_stream():
    """act, update_weights, act on a non-default stream: the first result is the old network's, the second the new one's."""
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    n = 65536                                                          # a kernel long enough to be running when the copy is enqueued
    obs = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, size=(n, 17)).astype(np.float32)).to(DEV)
    pol = _make_policy("shipped")
    old = pol.act(obs, deterministic=True).clone()
    new_weights = _perturbed(_make_policy("shipped"), seed=8)
    fresh = MlpPolicy(new_weights, seed=3).to(DEV)
    new = fresh.act(obs, deterministic=True).clone()
    assert not torch.equal(old, new)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    a, b = torch.empty_like(old), torch.empty_like(old)
    with torch.cuda.stream(side):
        pol.act(obs, deterministic=True, out=a)
        pol.update_weights(new_weights)
        pol.act(obs, deterministic=True, out=b)
    side.synchronize()
    assert torch.equal(a, old) and torch.equal(b, new)
    pol.close(); fresh.close()

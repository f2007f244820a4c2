"""
GPU tests (run with `-m gpu`) of the MLP actor and critic of other architectures than the shipped one (csrc/rdv_policy_mlp.h,
rdv_policy_create_mlp / rdv_critic_create_mlp in include/rdv.h) against the float64 NumPy reference of
tests/policy_mlp_reference.py: 1..4 hidden layers of 16 / 32 / 64, tanh / ReLU / sigmoid.

Deterministic bound, per (architecture, activation, network class, input set), actor and critic, entrywise form:
    e_hip = max|kernel - clip(mlp64)|  <=  1.5 e32 + A,      e32 = max|mlp32 - mlp64| (a property of the reference alone),
    a_0 = 6e-8,  a_l = Lip (|W_l| a_{l-1}) + d_act + 6e-8,  A = max(|W_head| a_L)       (policy_mlp_reference.error_floor_entrywise)
with d_tanh = 2.5e-7, d_relu = 0, d_sigmoid = 2.0e-7 (the header's derived bound) and Lip = 1, 1, 1/4.  The reference applies the
+-63 input clamp and the [0, 63] clamp of hidden ReLU activations, the kernels' two documented deviations from PyTorch.
Batch sizes 1 .. 1000 around the 32-env wave tile and the 256-env workgroup.
"""
import ctypes as C
import math

import numpy as np
import pytest

import policy_mlp_reference as M
import policy_reference as R
from helpers import gpu_batch
from policy_set_cases import DEV, act_via_abi as _act_handle, dev as _dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _policy(net, critic=None, seed=0):
    """An MlpPolicy (HIP backend) holding `net` as its actor and `critic` (default: the class's out_dim = 1 twin) as its critic;
    the architectures are inferred from the weights."""
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    p = MlpPolicy(M.weights_dict(net, M.critic_of(net) if critic is None else critic), activation_fn=net["act"]).to(DEV)
    p.noise_seed = seed
    return p


def _act(pol, obs, **kw):
    """rdv_policy_act through the C ABI with every noise argument given explicitly."""
    return _act_handle(pol._hip_handle(torch.device(DEV)), obs, **kw).cpu().numpy()


def _value(pol, obs):
    return pol.value(_dev(obs)).cpu().numpy()


@pytest.fixture(scope="module")
def input_sets():
    return M.input_sets()


@pytest.mark.parametrize("arch,act", M.all_cases(), ids=[f"{M.arch_id(a)}-{f}" for a, f in M.all_cases()])
def test_means_and_values_against_fp64(arch, act, input_sets):
    """Every architecture of the sweep (3 x 3 x 3) plus [64], [16], [64, 32, 16], [16, 64] with each activation; four network
    classes; actor and critic; every input set.  The classes' conditions (half of the outputs unclipped, ReLU below its clamp)
    are asserted on the CPU by tests/test_policy_mlp.py."""
    failures = []
    worst = {"actor": [0.0, 0.0, 0.0, 0.0, ""], "critic": [0.0, 0.0, 0.0, 0.0, ""]}
    for cid, make in M.CLASSES.items():
        net = make(arch, act)
        critic = M.critic_of(net)
        pol = _policy(net, critic)
        assert not pol.shipped_arch or act == "tanh"
        for sname, obs in input_sets.items():
            x = R.clamp_obs(obs)
            for kind, nn in (("actor", net), ("critic", critic)):
                y64, e32, a_entry = M.bounds(nn, x)
                if kind == "actor":
                    got, want = _act(pol, obs), np.clip(y64, -1.0, 1.0)
                else:
                    got, want = _value(pol, obs)[:, None], y64
                assert got.shape == want.shape and got.dtype == np.float32
                assert np.isfinite(got).all(), (cid, sname, kind)
                err = np.abs(got.astype(np.float64) - want)
                e_hip, bound = float(err.max()), 1.5 * e32 + a_entry
                if e_hip / bound >= worst[kind][3]:
                    worst[kind] = [e_hip, e32, a_entry, e_hip / bound, f"{cid}/{sname}"]
                if not e_hip <= bound:
                    failures.append((cid, sname, kind, e_hip, e32, a_entry, "row", int(err.max(axis=1).argmax())))
        pol.close()
    for kind, w in worst.items():
        print(f"TABLE {M.arch_id(arch):12s} {act:8s} {kind:6s} e_hip {w[0]:.3g}  e32 {w[1]:.3g}  A {w[2]:.3g}  ({w[4]}: {w[3]:.2f} of its bound)")
    assert not failures, failures


@pytest.mark.parametrize("act", M.ACTS)
@pytest.mark.parametrize("arch", M.ROUTE_ARCHS, ids=M.arch_id)
def test_routing_probes_reach_every_unit_of_every_layer(arch, act):
    """Sparse one-path networks: over route_nets(arch) of them every hidden index of every layer lies on a checked path (asserted on
    the CPU, test_policy_mlp.py); compared with the scalar fp64 composition, a failure names the path's unit in every layer."""
    obs = R.distinct_rows(257, seed=8)
    failures = []
    for m in range(M.route_nets(arch)):
        net, path = M.route_probe(arch, act, m)
        pol = _policy(net)
        got = _act(pol, obs)
        _, e32, a_entry = M.bounds(net, R.clamp_obs(obs))
        s64 = M.route_scalar64(net, path, obs)
        assert (np.abs(s64) < 1.0).all()                       # the clip plays no part
        # one-path networks leave e32 at an ulp or two and, for ReLU, A at 6e-8: what remains is the precision of the operands, two
        # fp16 terms = 22 bits (policy_mlp_reference.operand_floor, from the format and the reference's activations; measured on an
        # MI355X on [32] ReLU: 1.2e-7 at an output of 0.6, reproduced bit for bit by a NumPy emulation of the split).  A wrong fragment order
        # or padded tile moves an output by O(0.1).
        tol = 1.5 * e32 + a_entry + M.operand_floor(net, R.clamp_obs(obs))
        assert tol < 5e-6, tol
        for r, c in np.argwhere(np.abs(got - s64) > tol)[:4]:
            failures.append((m, M.describe_path(path, c), "row", int(r), float(got[r, c]), float(s64[r, c])))
        pol.close()
    assert not failures, failures


def test_relu_hidden_activations_are_clamped_to_63():
    """rdv.h, the second deviation from PyTorch: a first-layer unit that reaches 62.9, 63, 64 and 1e4 on chosen rows enters the next
    layer as min(., 63).  The unclamped network differs on the last two rows by far more than the bound (from the reference)."""
    net = M.relu_clamp_net()
    critic = M.critic_of(net)
    x, at = M.relu_clamp_rows()
    pol = _policy(net, critic)
    for kind, nn, got in (("actor", net, _act(pol, x)), ("critic", critic, _value(pol, x)[:, None])):
        y64, e32, a_entry = M.bounds(nn, R.clamp_obs(x))
        free = M.mlp64(nn, R.clamp_obs(x), clamp=False)
        want = np.clip(y64, -1.0, 1.0) if kind == "actor" else y64
        bound = 1.5 * e32 + a_entry
        assert np.abs(got - want).max() <= bound, (kind, np.abs(got - want).max(), bound)
        if kind == "critic":
            d = np.abs(free - y64)[at, 0]                      # 62.9 and 63: the clamp changes nothing; 64 and 1e4: it does
            assert d[:2].max() <= 1e-6 and d[2] > 10 * bound and d[3] > 1000 * bound, (d, bound)
    pol.close()


@pytest.mark.parametrize("act", M.ACTS)
def test_a_nan_row_poisons_only_itself(act):
    """A NaN observation gives NaN actions (value) for ITS row; every other row is bit-identical to the run without it."""
    net = M.dense([64, 16], act)
    pol = _policy(net, M.critic_of(M.dense([16, 32, 64], act, seed=4)))
    obs = R.distinct_rows(256, seed=77)
    a0, v0 = _act(pol, obs), _value(pol, obs)
    assert np.isfinite(a0).all() and np.isfinite(v0).all()
    for r, k in ((0, 0), (31, 16), (32, 7), (255, 12)):
        bad = obs.copy(); bad[r, k] = np.nan
        a, v = _act(pol, bad), _value(pol, bad)
        keep = np.arange(256) != r
        assert np.isnan(a[r]).all() and np.isnan(v[r]), (r, k, a[r], v[r])
        np.testing.assert_array_equal(a[keep], a0[keep], err_msg=f"actor, NaN in row {r}")
        np.testing.assert_array_equal(v[keep], v0[keep], err_msg=f"critic, NaN in row {r}")
    pol.close()


# ------------------------------------------------------------------------------------------------------------- the noise
def _noise_net():
    return dict(M.dense([32, 32, 32], "relu", seed=41), log_std=np.asarray((-5.0, -0.5, 0.0, 1.0, -0.5, 0.0), np.float32))


def _check_samples(tag, net, obs, raw, lp, clipped, seed, ids, counter):
    """test_gpu_policy_reference._check_samples with this module's reference network."""
    mean64, e32, a_entry = M.bounds(net, R.clamp_obs(obs))
    std = np.exp(net["log_std"].astype(np.float64))
    z = R.actor_normals(seed, ids, counter)
    want = mean64 + std * z
    tol = 1.5 * e32 + a_entry + std * R.TOL_Z
    if raw is not None:
        err = np.abs(raw.astype(np.float64) - want)
        assert (err <= tol).all(), (tag, "unclipped sample", float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())
    if clipped is not None:
        far = (np.abs(want - 1.0) > tol) & (np.abs(want + 1.0) > tol)
        err = np.abs(clipped.astype(np.float64) - np.clip(want, -1.0, 1.0))
        assert far.mean() > 0.9 and (err[far] <= np.broadcast_to(tol, err.shape)[far]).all(), (tag, "clipped sample", float(err[far].max()))
        assert (np.abs(clipped) <= 1.0).all()
    if lp is not None:
        lp64 = R.log_prob64(z, net["log_std"])
        tol_lp = 6.0 * np.abs(z).max(axis=1) * R.TOL_Z + 4e-6 * (1.0 + np.abs(lp64))
        err = np.abs(lp.astype(np.float64) - lp64)
        assert (err <= tol_lp).all(), (tag, "log_prob", float((err / tol_lp).max()))


def test_noise_of_another_architecture_against_philox_reference():
    """[32, 32, 32] ReLU with a non-zero log_std, n = 33: clipped samples of rdv_policy_act(deterministic = 0), unclipped actions
    and log_prob of rdv_rollout, against mean64 + exp(log_std) z_ref and log_prob64 with the six (seed, offset, counter) cases
    and the tolerances of test_gpu_policy_reference.py."""
    from test_gpu_policy_reference import CASES
    net = _noise_net()
    obs = R.distinct_rows(33, seed=5)
    n, T = 33, 2
    for seed, off, ctr in CASES:
        pol = _policy(net, seed=seed)
        ids = (off + np.arange(n)).astype(np.uint64)
        got = _act(pol, obs, deterministic=False, seed=seed, counter=ctr, offset=off)
        _check_samples(("act", hex(seed), off, ctr), net, obs, None, None, got, seed, ids, ctr)
        env = gpu_batch(n, seed=3, env_id_offset=off)
        env.reset()
        pol._calls = ctr                               # rdv_rollout's noise_counter0
        ro = env.rollout(pol, T)
        assert not env.last_kernel.startswith("rollout_kernel")
        for t in range(T):
            _check_samples(("rollout", hex(seed), off, ctr, t), net, ro["obs"][t].cpu().numpy(), ro["actions"][t].cpu().numpy(),
                           ro["log_prob"][t].cpu().numpy(), None, seed, ids, ctr + t)
        det = env.rollout(pol, 1, deterministic=True)
        const = -(float(net["log_std"].astype(np.float64).sum()) + 3.0 * math.log(2.0 * math.pi))
        assert float((det["log_prob"].double() - const).abs().max()) < 1e-5
        env.close(); pol.close()


# -------------------------------------------------------------------------------------------------- rollout: the definition
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("n", [33, 300])
def test_rollout_is_the_act_plus_step_loop(n, storage):
    """rdv.h: with a policy of another architecture rdv_rollout's results are those of rdv_policy_act(counter0 + t) followed by
    rdv_step.  batch.rollout(policy, 3) of a sigmoid [16, 16] policy against this test's own loop on a second batch of the same
    seed: obs, clipped actions, reward, done, last_obs, state and statistics bit for bit.  rdv_policy_act returns neither the
    unclipped sample nor its log-density: those rows are compared, bit for bit, with three one-step rollouts of a third batch, the
    unclipped sample where it lies inside the Box with the loop's clipped one (the clamp comparison), and log_prob with the
    shipped architecture's rollout kernel under the same log_std and noise key."""
    T, seed, ctr0, off = 3, 99, 5, 1000
    net = dict(M.dense([16, 16], "sigmoid", seed=43), log_std=np.asarray((-1.0, -0.5, 0.0, 0.5, -2.0, 0.2), np.float32))
    pol = _policy(net, seed=seed)
    envs = [gpu_batch(n, seed=7, storage=storage, env_id_offset=off) for _ in range(3)]
    for e in envs:
        e.reset()
    a, b, c = envs
    pol._calls = ctr0
    ro = a.rollout(pol, T)
    assert not a.last_kernel.startswith("rollout_kernel") and a.last_kernel.startswith("step_kernel")
    assert pol._calls == ctr0 + T
    handle = pol._hip_handle(torch.device(DEV))
    obs = b.obs.clone()
    for t in range(T):
        assert torch.equal(ro["obs"][t], obs), t
        act = _act_handle(handle, obs.contiguous(), deterministic=False, seed=seed, counter=ctr0 + t, offset=off)
        assert torch.equal(ro["actions"][t].clamp(-1.0, 1.0), act), t
        o, r, d = b.step(act)
        assert torch.equal(ro["reward"][t], r) and torch.equal(ro["done"][t].bool(), d.bool()), t
        obs = o.clone()
    assert torch.equal(ro["last_obs"], obs)
    pol._calls = ctr0
    for t in range(T):
        one = c.rollout(pol, 1)
        assert torch.equal(one["actions"][0], ro["actions"][t]) and torch.equal(one["log_prob"][0], ro["log_prob"][t]), t
    # log_prob is a function of (seed, env id, counter, log_std) alone: the shipped architecture's kernels (the persistent rollout
    # kernel here), pinned by test_gpu_policy_reference.py, give the same bits for the same log_std whatever their means are
    from helpers import shipped_policy
    ship = shipped_policy(device=DEV, noise_seed=seed)
    with torch.no_grad():
        ship.log_std.copy_(torch.from_numpy(net["log_std"]))
    d = gpu_batch(n, seed=7, storage=storage, env_id_offset=off)
    d.reset()
    ship._calls = ctr0
    rs = d.rollout(ship, T)
    assert d.last_kernel.startswith("rollout_kernel") and torch.equal(rs["log_prob"], ro["log_prob"])
    d.close(); ship.close()
    for other in (b, c):
        assert torch.equal(a.get_state(), other.get_state())
        assert a.get_stats() == other.get_stats()
    for e in envs:
        e.close()
    pol.close()


# --------------------------------------------------------------------------------- the default architecture, the new call
def test_default_spec_through_the_new_call_is_the_old_call():
    """rdv_policy_create_mlp / rdv_critic_create_mlp with the default spec and the shipped weights: bit-identical actions, values and
    3-step rollout to rdv_policy_create / rdv_critic_create, the persistent rollout kernel, and the default spec read back from a
    handle of either kind."""
    from reinforcement_learning_rendezvous_amd import _native as N
    from helpers import shipped_policy
    lib, n = N.lib(), 257
    old = shipped_policy(device=DEV, noise_seed=17)
    new = shipped_policy(device=DEV, noise_seed=17)
    spec = N.MlpSpec()
    N.check(lib.rdv_mlp_spec_default(C.byref(spec)))
    host = lambda t: t.detach().to("cpu", torch.float32).contiguous()
    for prefix, store in (("l", new._hip), ("v", new._hip_critic)):
        layers = new._layers(prefix)
        ws, bs = [host(l.weight) for l in layers], [host(l.bias) for l in layers]
        wp, bp = (C.c_void_p * 3)(*[t.data_ptr() for t in ws]), (C.c_void_p * 3)(*[t.data_ptr() for t in bs])
        h = C.c_void_p()
        if prefix == "l":
            ls = host(new.log_std)
            N.check(lib.rdv_policy_create_mlp(C.byref(spec), wp, bp, C.c_void_p(ls.data_ptr()), 0, C.byref(h)))
        else:
            N.check(lib.rdv_critic_create_mlp(C.byref(spec), wp, bp, 0, C.byref(h)))
        store[0] = h                                    # the policy object now launches through the handle of the new call
    got = N.MlpSpec()
    for h in (old._hip_handle(torch.device(DEV)), new._hip[0], new._hip_critic[0]):
        N.check(lib.rdv_policy_get_spec(h, C.byref(got)))
        assert got.to_tuple() == (2, [64, 64, 0, 0], N.ACT_TANH)
    obs = _dev(R.distinct_rows(n, seed=12))
    for det in (True, False):
        a_old = _act_handle(old._hip_handle(obs.device), obs, deterministic=det, seed=17, counter=3, offset=11)
        a_new = _act_handle(new._hip[0], obs, deterministic=det, seed=17, counter=3, offset=11)
        assert torch.equal(a_old, a_new)
    assert torch.equal(old.value(obs), new.value(obs))
    rows = {}
    for name, pol in (("old", old), ("new", new)):
        env = gpu_batch(n, seed=5)
        env.reset()
        pol._calls = 0
        rows[name] = env.rollout(pol, 3)
        assert env.last_kernel.startswith("rollout_kernel"), env.last_kernel
        rows[name]["state"] = env.get_state()
        env.close()
    for k in rows["old"]:
        assert torch.equal(rows["old"][k], rows["new"][k]), k
    old.close(); new.close()


# -------------------------------------------------------------------------------------------------------- other callers
def test_handles_of_the_new_kind_are_refused_where_the_old_ones_are():
    from reinforcement_learning_rendezvous_amd import _native as N
    pol = _policy(M.dense([32, 16], "relu"))
    obs = _dev(R.distinct_rows(8, seed=1))
    pol.value(obs)
    actor, critic = pol._hip_handle(obs.device), pol._hip_critic[0]
    spec = N.MlpSpec()
    N.check(N.lib().rdv_policy_get_spec(critic, C.byref(spec)))
    assert spec.to_tuple() == (2, [32, 16, 0, 0], N.ACT_RELU)
    out = torch.empty((8, 6), dtype=torch.float32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
    rc = N.lib().rdv_policy_act(critic, C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), 8, 1, 0, 0, 0, stream)
    assert rc == -1 and b"critic" in N.lib().rdv_last_error()
    rc = N.lib().rdv_policy_value(actor, C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), 8, stream)
    assert rc == -1 and b"actor" in N.lib().rdv_last_error()
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    wide = MlpPolicy(net_arch=[128, 128]).to(DEV)          # the PyTorch modules hold it; the kernels refuse it, naming the field
    with pytest.raises(N.RdvError, match=r"hidden\[0\] = 128"):
        wide.act(obs)
    assert wide.backend == "auto" and MlpPolicy(net_arch=[128, 128], backend="torch").to(DEV).act(obs).shape == (8, 6)
    pol.close()


def test_monte_carlo_run_takes_a_policy_of_another_architecture():
    """A smoke check of the caller path (no parity claim): monte_carlo.run with a [32, 32] ReLU policy on 256 initial conditions."""
    from helpers import load_golden
    from reinforcement_learning_rendezvous_amd import monte_carlo
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    pol = MlpPolicy(net_arch=[32, 32], activation_fn="relu", seed=3)
    ics = load_golden("mc_initial_conditions.npz")["states"][:256]
    res = monte_carlo.run(pol, ics, device=DEV)
    assert sorted(res) == sorted(monte_carlo.COLUMNS) and len(res) == 12
    assert all(v.shape == (256,) for v in res.values()) and (res["ep_len"] >= 1).all() and np.isfinite(res["total_reward"]).all()
    assert pol._calls >= 60 and 0 in pol._hip
    pol.close()

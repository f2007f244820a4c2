"""
GPU tests (run with `-m gpu`) of policy sets (include/rdv.h: one batch, several actors and critics, one launch; csrc/rdv_policy_sets.h).
The specification is one sentence — row i of member g gets bit for bit what a stand-alone handle of member g's weights computes for
that row, with the same seed, the same counter and env_id_offset + start_g — so a set is compared with stand-alone MlpPolicy objects
and separate batches, assert_array_equal throughout.  The reference is the existing single-policy path, which the other test files pin
to fp64 references and to the oracle; never the code under test.

Layouts, the smallest that hit every boundary: 968 rows as [256, 512, 200] (one tile, two tiles, a ragged last tile whose last wave
has 8 live lanes) and 549 rows as [256, 293] (a last wave of 37 live lanes; 549 % 4 = 1, so every row block of the critic after the
first starts off the 16-byte grid: the alignment case).  Architectures: the shipped [64, 64] tanh (member 0: the shipped checkpoint),
[32, 16] ReLU, [16] sigmoid, [64, 32, 16] tanh — both shipped-block kernels and all six instantiations of the general one.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_mlp_reference as M
from helpers import capture, gpu_batch, load_golden, persistent_kernel, to_numpy
from policy_set_cases import COLUMNS, DEV, assert_columns_equal, close as _close, env_sets as _env_sets, starts as _starts
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd import monte_carlo
from reinforcement_learning_rendezvous_amd._native import RdvError

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LAYOUTS = {"968": [256, 512, 200], "549": [256, 293]}
ARCHS = [([64, 64], "tanh"), ([32, 16], "relu"), ([16], "sigmoid"), ([64, 32, 16], "tanh")]
ARCH_IDS = [f"{M.arch_id(a)}-{f}" for a, f in ARCHS]
SEED = 5


@functools.lru_cache(maxsize=None)
def _member_weights(arch, act, g):
    """Member g of an (arch, act) set as a weights dict: distinct actor and critic networks per member, non-zero log_std; member 0 of
    the shipped architecture is the shipped checkpoint.  Computed once per (arch, act, g) and shared."""
    if g == 0 and list(arch) == [64, 64] and act == "tanh":
        return dict(load_golden("mlp_policy.npz"))
    net = M.dense(list(arch), act, seed=40 + g)
    net["log_std"] = np.random.default_rng(900 + g).uniform(-1.4, -0.4, 6).astype(np.float32)
    return M.weights_dict(net, M.critic_of(M.dense(list(arch), act, seed=70 + g)))


def _members(arch, act, count, shift=0):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    out = []
    for g in range(count):
        p = MlpPolicy(_member_weights(tuple(arch), act, g + shift), activation_fn=act).to(DEV)
        p.noise_seed = SEED
        assert p.has_critic
        out.append(p)
    return out


def _set(arch, act, sizes):
    from reinforcement_learning_rendezvous_amd import PolicySet
    members = _members(arch, act, len(sizes))
    return PolicySet(members, sizes), _members(arch, act, len(sizes))      # the set's members, and stand-alone twins of them


@functools.lru_cache(maxsize=None)
def _obs_host(shape, seed):
    """random observations in the Box [-1, 1]"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def _obs(*shape, seed=1):
    return torch.from_numpy(_obs_host(tuple(shape), seed)).to(DEV)


def _assert_members_differ(twins, obs):
    """two members give different outputs on the same observation: equality with the stand-alone handles below cannot hold by accident
    when a tile reads the wrong block"""
    rows = obs[:64].contiguous()
    a0, a1 = (to_numpy(p.act(rows, deterministic=True)) for p in twins[:2])
    v0, v1 = (to_numpy(p.value(rows)) for p in twins[:2])
    assert (a0 != a1).mean() > 0.9 and (v0 != v1).mean() > 0.9
    for p in twins[:2]:
        p._calls = 0


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("arch,act", ARCHS, ids=ARCH_IDS)
def test_act_equals_the_members_stand_alone(arch, act, layout):
    sizes = LAYOUTS[layout]
    pset, twins = _set(arch, act, sizes)
    n = sum(sizes)
    obs = _obs(n, 17, seed=int(layout))
    _assert_members_differ(twins, obs)
    assert len(pset) == len(sizes) and pset.num_rows == n and [(s.start, s.stop) for s in pset.group_slices] == [(a, a + m) for a, m in zip(_starts(sizes), sizes)]
    h = pset._hip_handle(torch.device(DEV))
    assert N.lib().rdv_policy_num_members(h) == len(sizes) and N.lib().rdv_policy_num_rows(h) == n
    plain = twins[0]._hip_handle(torch.device(DEV))
    assert N.lib().rdv_policy_num_members(plain) == 1 and N.lib().rdv_policy_num_rows(plain) == 0
    for deterministic in (True, False):
        for call in range(2):                                   # two successive calls: the counter advances
            assert pset._calls == twins[0]._calls
            got = to_numpy(pset.act(obs, deterministic=deterministic, env_id_offset=1000))
            want = np.concatenate([to_numpy(p.act(obs[s].contiguous(), deterministic=deterministic, env_id_offset=1000 + s.start))
                                   for p, s in zip(twins, pset.group_slices)])
            np.testing.assert_array_equal(got, want, err_msg=f"deterministic={deterministic}, call {call}")
            if not deterministic and call:
                assert (got != first).mean() > 0.5               # the counter really advanced
            first = got
    _close(pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("arch,act", ARCHS, ids=ARCH_IDS)
def test_value_over_row_blocks_equals_the_members_on_their_columns(arch, act, layout):
    """obs [3, n, 17]: row block y starts at flat row y * n; with n = 549 blocks 1 and 2 start 4 and 8 bytes off the 16-byte grid"""
    sizes = LAYOUTS[layout]
    pset, twins = _set(arch, act, sizes)
    n = sum(sizes)
    obs = _obs(3, n, 17, seed=10 + int(layout))
    _assert_members_differ(twins, obs[0])
    got = to_numpy(pset.value(obs))
    assert got.shape == (3, n)
    for p, s in zip(twins, pset.group_slices):
        np.testing.assert_array_equal(got[:, s], to_numpy(p.value(obs[:, s, :])), err_msg=f"member rows {s}")
    np.testing.assert_array_equal(to_numpy(pset.value(obs[1].clone())), got[1])  # [n, 17]: one row block (a copy: obs[1] itself starts off the 16-byte grid, which the ABI refuses)
    _close(pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 3
def _collect_equals_separate(env, parts, pset, twins, what):
    """one collect (the env parameter sets: policy_set_cases.env_sets) against separate batches and policies"""
    env.reset()
    [e.reset() for e in parts]
    got = env.collect(pset, 16, gamma=0.99, gae_lambda=0.95)
    want = [e.collect(p, 16, gamma=0.99, gae_lambda=0.95) for e, p in zip(parts, twins)]
    assert int(got["done"].sum(dim=0).min()) >= 1, "every env resets at least once"
    assert_columns_equal(got, want, what)
    assert pset._calls == 16 and all(p._calls == 16 for p in twins)
    return got


@pytest.mark.parametrize("arch,act,storage", [([64, 64], "tanh", "f32"), ([32, 16], "relu", "f32"), ([64, 64], "tanh", "f64")],
                         ids=["64x64-tanh-f32", "32x16-relu-f32", "64x64-tanh-f64"])
def test_collect_on_a_grouped_batch_equals_separate_batches_and_policies(arch, act, storage):
    sizes = LAYOUTS["968"]
    pset, twins = _set(arch, act, sizes)
    env = gpu_batch(sum(sizes), params=_env_sets(), group_sizes=sizes, storage=storage, seed=11)
    parts = [gpu_batch(m, params=p, env_id_offset=s, storage=storage, seed=11) for p, s, m in zip(_env_sets(), _starts(sizes), sizes)]
    _collect_equals_separate(env, parts, pset, twins, f"grouped {storage}")
    _close(env, parts, pset, twins)


@pytest.mark.parametrize("arch,act", [([64, 64], "tanh"), ([16], "sigmoid")], ids=["64x64-tanh", "16-sigmoid"])
def test_collect_on_an_ungrouped_batch_of_549_envs_with_two_members(arch, act):
    """a seed or hyper-parameter sweep on one env configuration: the handle has no parameter groups, the set two members"""
    sizes = LAYOUTS["549"]
    pset, twins = _set(arch, act, sizes)
    params = _env_sets()[1]
    env = gpu_batch(sum(sizes), params=params, seed=12)
    parts = [gpu_batch(m, params=params, env_id_offset=s, seed=12) for s, m in zip(_starts(sizes), sizes)]
    assert env.num_groups == 0
    _collect_equals_separate(env, parts, pset, twins, "ungrouped")
    assert "rollout_kernel" not in env.last_kernel and env.last_kernel != persistent_kernel("rollout", "f32"), env.last_kernel
    if arch == [64, 64]:
        assert parts[0].last_kernel == persistent_kernel("rollout", "f32")      # the stand-alone shipped policy took the one-launch form
    _close(env, parts, pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("arch,act", [([64, 64], "tanh"), ([64, 32, 16], "tanh")], ids=["64x64-tanh", "64x32x16-tanh"])
def test_refresh_of_one_member(arch, act):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    sizes = LAYOUTS["968"]
    pset, twins = _set(arch, act, sizes)
    n, s1 = sum(sizes), slice(256, 768)
    obs, obs3 = _obs(n, 17, seed=31), _obs(2, n, 17, seed=32)
    new = _member_weights(tuple(arch), act, 7)
    fresh = MlpPolicy(new, activation_fn=act).to(DEV)
    fresh.noise_seed = SEED
    before_a, before_v = to_numpy(pset.act(obs, deterministic=False)), to_numpy(pset.value(obs3))
    torch.cuda.synchronize()
    # queued in front of the refresh on the same stream: the old weights; behind it: the new ones (no synchronisation in between)
    pset._calls = 0
    queued_a, queued_v = pset.act(obs, deterministic=False), pset.value(obs3)
    pset.update_weights(member=1, weights=new)
    pset._calls = 0
    after_a, after_v = to_numpy(pset.act(obs, deterministic=False)), to_numpy(pset.value(obs3))
    np.testing.assert_array_equal(to_numpy(queued_a), before_a)
    np.testing.assert_array_equal(to_numpy(queued_v), before_v)
    want_a = to_numpy(fresh.act(obs[s1].contiguous(), deterministic=False, env_id_offset=256))
    np.testing.assert_array_equal(after_a[s1], want_a)
    np.testing.assert_array_equal(after_v[:, s1], to_numpy(fresh.value(obs3[:, s1, :])))
    assert (after_a[s1] != before_a[s1]).mean() > 0.9 and (after_v[:, s1] != before_v[:, s1]).mean() > 0.9
    for s in (slice(0, 256), slice(768, n)):                    # the other members: bit-identical to before
        np.testing.assert_array_equal(after_a[s], before_a[s])
        np.testing.assert_array_equal(after_v[:, s], before_v[:, s])
    # the member module is the source of truth: it holds the new weights now
    np.testing.assert_array_equal(to_numpy(pset[1].l1.weight), np.asarray(new["mlp_extractor.policy_net.0.weight"], np.float32))
    # all members at once (None: the modules' current parameters are pushed): nothing changes
    pset.update_weights()
    pset._calls = 0
    np.testing.assert_array_equal(to_numpy(pset.act(obs, deterministic=False)), after_a)
    _close(pset, twins, fresh)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_collect_as_one_graph_equals_eager_and_refresh_is_refused_inside():
    """collect(set, 4, out=buf) recorded on one stream (helpers.capture: linear, no parallel branches) and replayed, against the eager
    call on a twin batch in the same state with the noise counter of the recording.  update_weights during the capture is refused —
    RDV_ERR_INVALID_ARGUMENT naming the stream capture — before it touches the stream: the capture ends normally."""
    sizes = LAYOUTS["968"]

    class Twin:
        def __init__(self):
            self.pset, self.twins = _set([64, 64], "tanh", sizes)
            self.env = gpu_batch(sum(sizes), params=_env_sets(), group_sizes=sizes, seed=13)
            self.env.reset()
            self.out, self.calls, self.refusal = None, 0, None

        def collect(self):
            self.pset._calls = min(self.calls, 1) * 4           # a replay repeats the counter of the recording (include/rdv.h)
            self.calls += 1
            if self is graphed and torch.cuda.is_current_stream_capturing():
                with pytest.raises(RdvError) as e:
                    self.pset.update_weights(member=1)
                rc = lib.rdv_policy_set_member_weights(self.pset._hip_handle(torch.device(DEV)), 1, wp, bp, lp, self.env._stream())
                self.refusal = (e.value, rc, lib.rdv_last_error().decode())
            self.out = self.env.collect(self.pset, 4, gamma=0.99, gae_lambda=0.95, out=self.out)
            return self.out
    graphed, eager = Twin(), Twin()
    lib = N.lib()
    ws, bs, log_std = graphed.pset[1]._host_layers("l")         # host copies made outside the capture
    wp, bp, lp = (C.c_void_p * 3)(*[t.data_ptr() for t in ws]), (C.c_void_p * 3)(*[t.data_ptr() for t in bs]), C.c_void_p(log_std[0].data_ptr())
    g = capture(graphed.collect)                                 # ends normally: torch raises if the capture was invalidated
    err, rc, message = graphed.refusal
    assert err.code == -1 and "stream capture" in str(err)
    assert rc == -1 and "stream capture" in message and message.startswith("rdv_policy_set_member_weights:"), (rc, message)
    eager.collect()
    for r in range(2):
        for t in graphed.out.values():
            t.fill_(0)                                           # the replay, not the recording's warm-up, wrote what is compared
        g.replay()
        want = eager.collect()
        torch.cuda.synchronize()
        for name in COLUMNS:
            np.testing.assert_array_equal(to_numpy(graphed.out[name]), to_numpy(want[name]), err_msg=f"{name}, replay {r}")
    np.testing.assert_array_equal(to_numpy(graphed.env.get_state()), to_numpy(eager.env.get_state()))
    assert graphed.env.get_stats() == eager.env.get_stats()
    for t in (graphed, eager):
        _close(t.env, t.pset, t.twins)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_refusals_name_the_numbers_and_leave_the_handles_usable():
    lib = N.lib()
    sizes = LAYOUTS["968"]
    n = sum(sizes)
    pset, twins = _set([32, 16], "relu", sizes)
    dev = torch.device(DEV)
    actor, critic = pset._hip_handle(dev), pset._critic_handle(dev)
    obs = _obs(n, 17, seed=41)
    before_a, before_v = to_numpy(pset.act(obs, deterministic=True)), to_numpy(pset.value(obs))
    out6, out1 = torch.empty((2 * n, 6), device=DEV), torch.empty((2 * n,), device=DEV)
    big = _obs(2 * n, 17, seed=42)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws, bs, log_std = pset[0]._host_layers("l")
    wp, bp, lp = (C.c_void_p * 3)(*[t.data_ptr() for t in ws]), (C.c_void_p * 3)(*[t.data_ptr() for t in bs]), C.c_void_p(log_std[0].data_ptr())

    def refused(rc, *needles):
        message = lib.rdv_last_error().decode()
        assert rc == -1, (rc, message)                         # RDV_ERR_INVALID_ARGUMENT
        for x in needles:
            assert str(x) in message, (x, message)

    # set rows != batch envs in rollout
    env = gpu_batch(512, params=_env_sets()[0], seed=14)
    env.reset()
    with pytest.raises(RdvError) as e:
        env.rollout(pset, 4)
    assert e.value.code == -1 and "968" in str(e.value) and "512" in str(e.value)
    # act with another n than the set's rows
    refused(lib.rdv_policy_act(actor, C.c_void_p(big.data_ptr()), C.c_void_p(out6.data_ptr()), 512, 1, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), stream), 512, 968)
    # value with n not a multiple of the rows
    refused(lib.rdv_policy_value(critic, C.c_void_p(big.data_ptr()), C.c_void_p(out1.data_ptr()), n + 256, stream), n + 256, 968)
    # rdv_rollout_advantages passes n through: half the rows twice over would satisfy "a multiple", and is refused by its own check
    half = n // 2
    cols = [torch.zeros((2, half), device=DEV) for _ in range(3)] + [torch.zeros((half,), device=DEV)]
    done = torch.zeros((2, half), dtype=torch.uint8, device=DEV)
    rows = N.RolloutOut(big.data_ptr(), None, cols[0].data_ptr(), done.data_ptr(), None, big.data_ptr())
    ao = N.AdvantageOut(cols[1].data_ptr(), cols[3].data_ptr(), cols[2].data_ptr(), out1.data_ptr())
    refused(lib.rdv_rollout_advantages(critic, C.byref(rows), 2, half, 0.99, 0.95, C.byref(ao), stream), half, 968)
    # rdv_policy_set_weights on a set: names the member call
    refused(lib.rdv_policy_set_weights(actor, wp, bp, lp, stream), "rdv_policy_set_member_weights", 3)
    # member index out of range
    refused(lib.rdv_policy_set_member_weights(actor, 3, wp, bp, lp, stream), "member 3 of 3")
    refused(lib.rdv_policy_set_member_weights(actor, -1, wp, bp, lp, stream), "member -1 of 3")
    # an actor set passed to value, a critic set passed to act
    refused(lib.rdv_policy_value(actor, C.c_void_p(obs.data_ptr()), C.c_void_p(out1.data_ptr()), n, stream), "actor")
    refused(lib.rdv_policy_act(critic, C.c_void_p(obs.data_ptr()), C.c_void_p(out6.data_ptr()), n, 1, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), stream), "critic")
    # Python's own check of the rows, before the library is asked
    with pytest.raises(ValueError, match="512 rows, the policy set owns 968"):
        pset.act(obs[:512].contiguous())
    # the handles are as usable as before
    np.testing.assert_array_equal(to_numpy(pset.act(obs, deterministic=True)), before_a)
    np.testing.assert_array_equal(to_numpy(pset.value(obs)), before_v)
    _close(env, pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_monte_carlo_sweep_with_one_policy_per_config():
    """two configs, two policies, 40 stored initial conditions (each group padded to 256 rows): every table equals monte_carlo.run of
    that config's policy, in all twelve columns"""
    ics = load_golden("mc_initial_conditions.npz")["states"][:40]
    configs = [dict(dt=1.0, t_max=12), dict(dt=0.5, t_max=8, koz_radius=4.0)]
    tables = monte_carlo.sweep(_members([64, 64], "tanh", 2), ics, configs, storage="f32")
    assert len(tables) == 2
    for c, (config, got) in enumerate(zip(configs, tables)):
        want = monte_carlo.run(_members([64, 64], "tanh", 2)[c], ics, storage="f32", config=config)
        for col in monte_carlo.COLUMNS:
            assert got[col].shape == (40,)
            np.testing.assert_array_equal(got[col], want[col], err_msg=f"{col}, config {c}")
    swapped = monte_carlo.run(_members([64, 64], "tanh", 2)[1], ics, storage="f32", config=configs[0])
    assert any((tables[0][col] != swapped[col]).any() for col in monte_carlo.COLUMNS)      # the policy of a config matters
    with pytest.raises(ValueError, match="3 policies for 2 configs"):
        monte_carlo.sweep(_members([64, 64], "tanh", 3), ics, configs)

"""
GPU tests (run with `-m gpu`) of recurrent policy sets (include/rdv.h, "Recurrent policy sets"; the set forms of the kernels of
csrc/rdv_policy_lstm.h).  The specification is one sentence — row i of member g gets bit for bit what a stand-alone recurrent handle of
member g's arrays with n_rows = sizes[g] computes for that row, fed the same observations and episode starts, with the same seed, the
same counter and env_id_offset + start_g, over any number of steps — so a set is compared with stand-alone LstmPolicy objects and
separate batches, by equality throughout: actions, samples, log-densities, values, and the state (h, c) after every call.  The
reference is the single-policy path, which tests/test_gpu_policy_lstm.py pins to the fp64 reference; never the code under test.

Layouts: (256, 256) two full tiles; (256, 37) a ragged last member of one full wave and 5 rows; (512, 256, 1) a member over two tiles
and a one-row last member.  Every member has its own actor, critic and log_std, so a tile that reads the wrong block cannot pass.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_lstm_reference as L
from helpers import gpu_batch, load_golden, to_numpy
from policy_set_cases import (DEV, assert_columns_equal, close as _close, dev as _dev, env_sets, lstm_loop, short_episodes as _short_episodes,
                              stagger as _stagger, starts as _starts, stream as _stream)
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd import monte_carlo
from reinforcement_learning_rendezvous_amd._native import RdvError

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LAYOUTS = {"256+256": (256, 256), "256+37": (256, 37), "512+256+1": (512, 256, 1)}
SEED = 0xABCDEF12345


@functools.lru_cache(maxsize=None)
def _member_weights(H, arch, act, g, cid="hot"):
    """Member g as a weights dict: a hot actor (the recursion matters), a critic of another seed, a non-zero log_std of its own.
    `cid`: another class of policy_lstm_reference.ALL_CLASSES for the actor AND the critic (a cell scale of its own)."""
    net = L.ALL_CLASSES[cid](H, arch, act, seed=51 + g)
    net = dict(net, log_std=np.random.default_rng(900 + g).uniform(-1.4, -0.4, 6).astype(np.float32))
    return L.weights_dict(net, L.critic_of((L.default_init if cid == "hot" else L.ALL_CLASSES[cid])(H, arch, act, seed=77 + g)))


def _member(H, arch, act, g, n_rows=None, offset=0, cid="hot"):
    from reinforcement_learning_rendezvous_amd import LstmPolicy
    p = LstmPolicy(_member_weights(H, tuple(arch), act, g, cid), activation_fn=act, n_rows=n_rows).to(DEV)
    p.noise_seed, p.noise_env_offset = SEED, offset
    return p


def _set(H, sizes, arch=(64, 64), act="tanh", shift=0, classes=None):
    """(the set, stand-alone twins of its members: n_rows = sizes[g], noise_env_offset = start_g, the same seed)"""
    from reinforcement_learning_rendezvous_amd import LstmPolicySet
    classes = classes or ("hot",) * len(sizes)
    pset = LstmPolicySet([_member(H, arch, act, g + shift, cid=classes[g]) for g in range(len(sizes))], sizes, seed=SEED)
    twins = [_member(H, arch, act, g + shift, n_rows=m, offset=s, cid=classes[g]) for g, (m, s) in enumerate(zip(sizes, _starts(sizes)))]
    return pset, twins


def _cat(parts):
    return torch.cat(list(parts), dim=0)


def _assert_state_equal(pset, twins, what):
    for name in ("state", "critic_state"):
        got = getattr(pset, name)
        want = [getattr(p, name) for p in twins]
        for i, hc in enumerate("hc"):
            assert torch.equal(got[i], _cat(w[i] for w in want)), f"{name} {hc}, {what}"


# ---------------------------------------------------------------------------------------------------------------- 1
def _act_and_value_equal_the_members(H, sizes, arch, act, classes=None):
    pset, twins = _set(H, sizes, arch, act, classes=classes)
    n = sum(sizes)
    obs, starts = L.obs_sequence(n, 4), L.episode_starts(n, 3)
    assert len(pset) == len(sizes) and pset.n_rows == n and [(s.start, s.stop) for s in pset.group_slices] == [(a, a + m) for a, m in zip(_starts(sizes), sizes)]
    for deterministic in (True, False):
        for t in range(3):
            what = f"deterministic={deterministic}, step {t}"
            o, s = _dev(obs[t]), starts[t]
            assert all(p._calls == pset._calls for p in twins)
            raw, lp = torch.empty((n, 6), dtype=torch.float32, device=DEV), torch.empty((n,), dtype=torch.float32, device=DEV)
            got = pset.act(o, episode_start=s, deterministic=deterministic, raw_out=raw, log_prob_out=lp)
            want = []
            for p, sl in zip(twins, pset.group_slices):
                r, q = torch.empty((sl.stop - sl.start, 6), dtype=torch.float32, device=DEV), torch.empty((sl.stop - sl.start,), dtype=torch.float32, device=DEV)
                a = p.act(o[sl].contiguous(), episode_start=s[sl], deterministic=deterministic, raw_out=r, log_prob_out=q)
                want.append((a, r, q))
            for i, name in enumerate(("actions", "raw_actions", "log_prob")):
                assert torch.equal((got, raw, lp)[i], _cat(w[i] for w in want)), f"{name}, {what}"
            v = pset.value(o, episode_start=s)
            assert torch.equal(v, _cat(p.value(o[sl].contiguous(), episode_start=s[sl]) for p, sl in zip(twins, pset.group_slices))), f"value, {what}"
            _assert_state_equal(pset, twins, what)
            if t == 0 and deterministic and len(sizes) > 1 and sizes[1] > 1:          # the members differ: the first rows of members 0 and 1 on one observation
                k = min(sizes[1], 32)
                same = o[:k].repeat(n // k + 1, 1)[:n].contiguous()
                probe, _ = _set(H, sizes, arch, act, classes=classes)
                a = probe.act(same, episode_start=np.ones(n, np.uint8))
                assert (to_numpy(a[:k]) != to_numpy(a[sizes[0]:sizes[0] + k])).mean() > 0.9
                probe.close()
    # a non-committing value on a fourth observation, and the state behind it
    before = pset.critic_state
    o = _dev(obs[3])
    peek = pset.value(o, commit=False)
    assert torch.equal(peek, _cat(p.value(o[sl].contiguous(), commit=False) for p, sl in zip(twins, pset.group_slices)))
    after = pset.critic_state
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert float(before[0].abs().max()) > 0.01
    h = pset._hip_handle(torch.device(DEV))
    assert N.lib().rdv_policy_num_members(h) == len(sizes) and N.lib().rdv_policy_num_rows(h) == n and N.lib().rdv_lstm_hidden_size(h) == H
    _close(pset, twins)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_act_and_value_equal_the_members_stand_alone(H, layout):
    _act_and_value_equal_the_members(H, LAYOUTS[layout], (64, 64), "tanh")


@pytest.mark.parametrize("arch,act", L.EXTRA_TRUNKS, ids=[f"{'x'.join(map(str, a))}-{f}" for a, f in L.EXTRA_TRUNKS])
def test_other_trunks_equal_the_members_stand_alone(arch, act):
    _act_and_value_equal_the_members(64, LAYOUTS["256+37"], tuple(arch), act)


def test_members_of_three_cell_scales_equal_the_members_stand_alone():
    """A block's cell header is relative to its member: members whose cells have the shifts 10, 3 (W_ih's) and 9 (W_hh's) in one set,
    the member of 33 rows last (every size but the last is a multiple of 256)."""
    classes = ("hot", "ih_shift3", "hh_shift9")
    assert [min(L.CLASS_SHIFTS[c]) for c in classes] == [10, 3, 9]
    _act_and_value_equal_the_members(64, (256, 256, 33), (64, 64), "tanh", classes=classes)


def test_a_set_of_one_member_equals_the_plain_handle():
    """n_members = 1 is legal: the plain kernels on the one block"""
    pset, twins = _set(64, (293,))
    obs, starts = L.obs_sequence(293, 2), L.episode_starts(293, 2)
    for t in range(2):
        assert torch.equal(pset.act(_dev(obs[t]), episode_start=starts[t], deterministic=False),
                           twins[0].act(_dev(obs[t]), episode_start=starts[t], deterministic=False))
    _assert_state_equal(pset, twins, "one member")
    _close(pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_state_calls_through_the_set():
    sizes = LAYOUTS["256+256"]
    pset, twins = _set(64, sizes)
    n = sum(sizes)
    obs, starts = L.obs_sequence(n, 3), L.episode_starts(n, 3)
    for t in range(2):
        pset.act(_dev(obs[t]), episode_start=starts[t]); pset.value(_dev(obs[t]), episode_start=starts[t])
        for p, sl in zip(twins, pset.group_slices):
            p.act(_dev(obs[t][sl]), episode_start=starts[t][sl]); p.value(_dev(obs[t][sl]), episode_start=starts[t][sl])
    mask = (np.arange(n) % 7 == 3).astype(np.uint8)
    h0, c0 = pset.state
    pset.reset_state(mask)
    for p, sl in zip(twins, pset.group_slices):
        p.reset_state(mask[sl])
    _assert_state_equal(pset, twins, "reset_state(mask)")
    m = torch.from_numpy(mask).to(DEV).bool()
    h1, c1 = pset.state
    assert (h1[m] == 0).all() and (c1[m] == 0).all() and torch.equal(h1[~m], h0[~m]) and torch.equal(c1[~m], c0[~m]) and float(h1.abs().max()) > 0.01
    # set / get: the state IS what the next step reads
    pset.state = (h0, c0)
    pset.critic_state = (c0, h0)
    assert torch.equal(pset.state[0], h0) and torch.equal(pset.state[1], c0) and torch.equal(pset.critic_state[0], c0)
    for p, sl in zip(twins, pset.group_slices):
        p.state = (h0[sl].contiguous(), c0[sl].contiguous())
        p.critic_state = (c0[sl].contiguous(), h0[sl].contiguous())
    o = _dev(obs[2])
    assert torch.equal(pset.act(o), _cat(p.act(o[sl].contiguous()) for p, sl in zip(twins, pset.group_slices)))
    assert torch.equal(pset.value(o), _cat(p.value(o[sl].contiguous()) for p, sl in zip(twins, pset.group_slices)))
    _assert_state_equal(pset, twins, "after set_state")
    pset.reset_state()
    assert float(pset.state[0].abs().max()) == 0.0 and float(pset.critic_state[1].abs().max()) == 0.0
    _close(pset, twins)


def test_refresh_of_one_member_and_the_refusal_of_the_whole_set_call():
    sizes = LAYOUTS["256+256"]
    pset, twins = _set(64, sizes)
    n = sum(sizes)
    obs, starts = L.obs_sequence(n, 3), L.episode_starts(n, 3)
    for t in range(2):
        pset.act(_dev(obs[t]), episode_start=starts[t], deterministic=False); pset.value(_dev(obs[t]), episode_start=starts[t])
    sl0, sl1 = pset.group_slices
    twins[0].act(_dev(obs[0][sl0]), episode_start=starts[0][sl0], deterministic=False); twins[0].value(_dev(obs[0][sl0]), episode_start=starts[0][sl0])
    twins[0].act(_dev(obs[1][sl0]), episode_start=starts[1][sl0], deterministic=False); twins[0].value(_dev(obs[1][sl0]), episode_start=starts[1][sl0])
    state, cstate = pset.state, pset.critic_state
    new = _member_weights(64, (64, 64), "tanh", 11)
    pset.update_weights(member=1, weights=new)
    for a, b in zip(state + cstate, pset.state + pset.critic_state):
        assert torch.equal(a, b)                                                          # the whole state is untouched
    fresh = _member(64, (64, 64), "tanh", 11, n_rows=sizes[1], offset=sizes[0])
    fresh.state = (state[0][sl1].contiguous(), state[1][sl1].contiguous())
    fresh.critic_state = (cstate[0][sl1].contiguous(), cstate[1][sl1].contiguous())
    fresh._calls = pset._calls
    o, s = _dev(obs[2]), starts[2]
    a, v = pset.act(o, episode_start=s, deterministic=False), pset.value(o, episode_start=s)
    assert torch.equal(a[sl1], fresh.act(o[sl1].contiguous(), episode_start=s[sl1], deterministic=False)) and torch.equal(v[sl1], fresh.value(o[sl1].contiguous(), episode_start=s[sl1]))
    assert torch.equal(a[sl0], twins[0].act(o[sl0].contiguous(), episode_start=s[sl0], deterministic=False)) and torch.equal(v[sl0], twins[0].value(o[sl0].contiguous(), episode_start=s[sl0]))
    _assert_state_equal(pset, [twins[0], fresh], "after the refresh of member 1")
    old = _member(64, (64, 64), "tanh", 1, n_rows=sizes[1], offset=sizes[0])            # ... and the new weights are not the old ones
    old.state = (state[0][sl1].contiguous(), state[1][sl1].contiguous())
    old._calls = pset._calls - 1
    assert not torch.equal(a[sl1], old.act(o[sl1].contiguous(), episode_start=s[sl1], deterministic=False))
    # rdv_lstm_set_weights on the set: refused, naming the member call; the set is as usable as before
    lib = N.lib()
    lstm, ws, bs, log_std = pset[0]._host_arrays("l")
    wp, bp = (C.c_void_p * 3)(*[t.data_ptr() for t in ws]), (C.c_void_p * 3)(*[t.data_ptr() for t in bs])
    rc = lib.rdv_lstm_set_weights(pset._hip[0], *[C.c_void_p(t.data_ptr()) for t in lstm], wp, bp, C.c_void_p(log_std[0].data_ptr()), _stream())
    message = lib.rdv_last_error().decode()
    assert rc == -1 and "rdv_lstm_set_member_weights" in message and "2 members" in message, message
    bad = dict(new); bad["lstm_critic.weight_ih_l0"] = new["lstm_critic.weight_ih_l0"].copy(); bad["lstm_critic.weight_ih_l0"][5, 5] = np.nan
    with pytest.raises(RdvError, match="non-finite"):
        pset.update_weights(member=0, weights=bad)
    _close(pset, twins, fresh, old)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_rollout_is_the_set_act_plus_step_loop_and_continues():
    """512 envs x 8 steps, episodes of 4 steps, a set of (256, 256): rdv_rollout with the set against the explicit loop on a clone —
    every column and last_obs by equality; two rollouts of 4 steps equal one of 8 (the second goes on from the pending flags)."""
    sizes, T, ctr0, off = LAYOUTS["256+256"], 8, 9, 700
    n = sum(sizes)
    env = gpu_batch(n, params=_short_episodes(), seed=13, env_id_offset=off)
    env.reset()
    _stagger(env)
    envs = [env, env.clone(), env.clone()]
    sets = [_set(64, sizes)[0] for _ in range(3)]
    sets[0]._calls = ctr0
    ro = envs[0].rollout(sets[0], T)
    assert envs[0].last_kernel.startswith("step_kernel") and sets[0]._calls == ctr0 + T
    assert int(ro["done"].sum()) >= n and int(ro["done"][:-1].sum()) > 0                  # episodes end inside the rollout
    loop, _ = lstm_loop(envs[1], sets[1], T, ctr0)
    for k in ("obs", "actions", "reward", "done", "log_prob", "last_obs"):
        assert torch.equal(ro[k].to(loop[k].dtype), loop[k]), k
    assert float(ro["lstm_state0"][0].abs().max()) == 0.0                                # every row was pending: step 0 starts from zero
    sets[2]._calls = ctr0
    first = envs[2].rollout(sets[2], T // 2)
    first = {k: (tuple(x.clone() for x in v) if isinstance(v, tuple) else v.clone()) for k, v in first.items()}
    mid_state = sets[2].state_at_start("l", DEV)
    second = envs[2].rollout(sets[2], T // 2)
    for k in ("obs", "actions", "reward", "done", "log_prob"):
        assert torch.equal(torch.cat([first[k], second[k]]), ro[k]), k
    assert torch.equal(second["last_obs"], ro["last_obs"])
    for x, y in zip(second["lstm_state0"], mid_state):
        assert torch.equal(x, y)
    keep = first["done"][-1] == 0
    assert 0 < int(keep.sum()) < n
    assert float(second["lstm_state0"][0][~keep].abs().max()) == 0.0 and float(second["lstm_state0"][0][keep].abs().max()) > 0.0
    for p in sets[1:]:
        for x, y in zip(p.state, sets[0].state):
            assert torch.equal(x, y)
    _close(envs, sets)


def _collect_equals_separate(env, parts, pset, twins, what, T=16):
    """two collects in a row (the second continues from the pending flags of actor and critic) against separate batches and policies"""
    env.reset()
    [e.reset() for e in parts]
    for call in range(2):
        got = env.collect(pset, T, gamma=0.99, gae_lambda=0.95)
        want = [e.collect(p, T, gamma=0.99, gae_lambda=0.95) for e, p in zip(parts, twins)]
        assert int(got["done"].sum(dim=0).min()) >= 1, "every env resets at least once"
        assert_columns_equal(got, want, f"{what}, call {call}", extra=("lstm_state0",))
        assert pset._calls == T * (call + 1) and all(p._calls == T * (call + 1) for p in twins)
    _assert_state_equal(pset, twins, what)


def test_collect_on_a_grouped_batch_equals_separate_batches_and_policies():
    sizes = LAYOUTS["256+256"]
    pset, twins = _set(64, sizes)
    for p in twins:
        p.noise_env_offset = 0                                   # the separate batches pass their env_id_offset = start_g themselves
    env = gpu_batch(sum(sizes), params=env_sets()[:2], group_sizes=list(sizes), seed=11)
    parts = [gpu_batch(m, params=p, env_id_offset=s, seed=11) for p, s, m in zip(env_sets()[:2], _starts(sizes), sizes)]
    assert env.num_groups == 2
    _collect_equals_separate(env, parts, pset, twins, "grouped")
    _close(env, parts, pset, twins)


def test_collect_on_an_ungrouped_batch_of_549_envs_with_two_members():
    """549 % 4 = 1: row t of [T, N, 17] is not 16-byte aligned, the critic set reads it through its aligned scratch rows; the last
    member has 293 rows (a tile of 37: one full wave and 5 rows)"""
    sizes = (256, 293)
    pset, twins = _set(32, sizes)
    params = env_sets()[1]
    env = gpu_batch(sum(sizes), params=params, seed=12)
    parts = [gpu_batch(m, params=params, env_id_offset=s, seed=12) for s, m in zip(_starts(sizes), sizes)]
    assert env.num_groups == 0
    _collect_equals_separate(env, parts, pset, twins, "ungrouped")
    _close(env, parts, pset, twins)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_monte_carlo_sweep_with_one_lstm_policy_per_config():
    """two configs, two recurrent policies, 24 stored initial conditions (each group padded to 256 rows): every table equals
    monte_carlo.run of that config's policy (a fresh one: zero state) in all twelve columns"""
    ics = load_golden("mc_initial_conditions.npz")["states"][:24]
    configs = [dict(dt=1.0, t_max=12), dict(dt=0.5, t_max=8, koz_radius=4.0)]
    members = lambda: [_member(64, (64, 64), "tanh", g) for g in range(2)]
    tables = monte_carlo.sweep(members(), ics, configs, storage="f32")
    assert len(tables) == 2
    for c, (config, got) in enumerate(zip(configs, tables)):
        pol = members()[c]
        want = monte_carlo.run(pol, ics, storage="f32", config=config)
        pol.close()
        for col in monte_carlo.COLUMNS:
            assert got[col].shape == (24,)
            np.testing.assert_array_equal(got[col], want[col], err_msg=f"{col}, config {c}")
    pol = members()[1]
    swapped = monte_carlo.run(pol, ics, storage="f32", config=configs[0])
    pol.close()
    assert any((tables[0][col] != swapped[col]).any() for col in monte_carlo.COLUMNS)      # the policy of a config matters
    with pytest.raises(ValueError, match="3 policies for 2 configs"):
        monte_carlo.sweep(members() + members()[:1], ics, configs)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_refusals_name_the_numbers_and_leave_the_handles_usable():
    lib = N.lib()
    sizes = LAYOUTS["256+37"]
    n = sum(sizes)
    pset, twins = _set(32, sizes)
    dev = torch.device(DEV)
    obs = _dev(L.obs_sequence(n, 1)[0])
    ones = np.ones(n, np.uint8)
    before_a, before_v = to_numpy(pset.act(obs, episode_start=ones)), to_numpy(pset.value(obs, episode_start=ones))
    actor, critic = pset._hip_handle(dev), pset._critic_handle(dev)
    big = _dev(L.obs_sequence(2 * n, 1)[0])
    out6, out1 = torch.empty((2 * n, 6), device=DEV), torch.empty((2 * n,), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    lstm, ws, bs, log_std = pset[0]._host_arrays("l")
    lp4 = [p(t) for t in lstm]
    wp, bp = (C.c_void_p * 3)(*[t.data_ptr() for t in ws]), (C.c_void_p * 3)(*[t.data_ptr() for t in bs])

    def refused(rc, *needles):
        message = lib.rdv_last_error().decode()
        assert rc == -1, (rc, message)                         # RDV_ERR_INVALID_ARGUMENT
        for x in needles:
            assert str(x) in message, (x, message)

    # n != the set's rows
    refused(lib.rdv_lstm_act(actor, p(big), None, p(out6), None, None, 256, 1, 0, 0, 0, _stream()), 256, n)
    refused(lib.rdv_lstm_value(critic, p(big), None, p(out1), 2 * n, 1, _stream()), 2 * n, n)
    with pytest.raises(ValueError, match=f"256 rows, the policy owns the state of {n}"):
        pset.act(obs[:256].contiguous())
    # rdv_rollout with rows != envs
    env = gpu_batch(512, seed=14)
    env.reset()
    with pytest.raises(ValueError, match="512 rows"):
        env.rollout(pset, 2)
    ro = N.RolloutOut(*[p(torch.empty(512 * 17 * 2, device=DEV)) for _ in range(6)])
    refused(lib.rdv_rollout(env._h, actor, 2, C.byref(ro), 1, 0, 0, _stream()), f"owns {n} rows", "512 envs")
    # member out of range
    refused(lib.rdv_lstm_set_member_weights(actor, 2, *lp4, wp, bp, p(log_std[0]), _stream()), "member 2 of 2")
    refused(lib.rdv_lstm_set_member_weights(actor, -1, *lp4, wp, bp, p(log_std[0]), _stream()), "member -1 of 2")
    with pytest.raises(IndexError, match="member 2 of 2"):
        pset.update_weights(member=2)
    # the MLP member call on the recurrent set
    refused(lib.rdv_policy_set_member_weights(actor, 0, wp, bp, p(log_std[0]), _stream()), "recurrent")
    refused(lib.rdv_policy_act(actor, p(obs), p(out6), n, 1, 0, 0, 0, _stream()), "recurrent")
    # an actor set passed to value, a critic set passed to act
    refused(lib.rdv_lstm_value(actor, p(obs), None, p(out1), n, 1, _stream()), "actor")
    refused(lib.rdv_lstm_act(critic, p(obs), None, p(out6), None, None, n, 1, 0, 0, 0, _stream()), "critic")
    # member 0 of a plain recurrent handle is the handle; member 1 is out of range
    twins[0].act(obs[:256].contiguous())
    refused(lib.rdv_lstm_set_member_weights(twins[0]._hip[0], 1, *lp4, wp, bp, p(log_std[0]), _stream()), "member 1 of 1")
    assert lib.rdv_lstm_set_member_weights(twins[0]._hip[0], 0, *lp4, wp, bp, p(log_std[0]), _stream()) == 0
    # the handles are as usable as before
    np.testing.assert_array_equal(to_numpy(pset.act(obs, episode_start=ones)), before_a)
    np.testing.assert_array_equal(to_numpy(pset.value(obs, episode_start=ones)), before_v)
    _close(env, pset, twins)

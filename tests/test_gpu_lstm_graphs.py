"""
GPU tests (run with `-m gpu`) of HIP-graph replay and stream order of the RECURRENT policy calls (include/rdv.h, "Stream capture"):
rdv_lstm_act, rdv_lstm_value, rdv_lstm_get_state / set_state / reset_state, rdv_rollout and rdv_rollout_advantages with an LSTM handle,
and the set forms.  The frame is tests/test_gpu_graphs.py's — two twins of one seed and weights, `graphed` records its calls once
(helpers.capture: one stream, a linear sequence, the calls made once eagerly first) and replays them, `eager` makes the same calls again
— and so is the specification: a replayed graph computes bit for bit what the same calls compute eagerly.  Every comparison is on bits
(`_equal`); the one exception is the reference check of section 1, at the tolerance of tests/test_gpu_policy_lstm.py.

What sets these calls apart is the state they carry from one call to the next, all of it on the device: (h, c), the pending
episode-start flags, and the scratch rows h_next, c_tmp and obs_tmp.  A replay has to pick that state up from the device, not from the
recording.  So the rollouts run T = 6 steps over episodes of 4 (policy_set_cases.short_episodes behind stagger): done[T-1], the flags a
call leaves pending, is a strict, non-empty subset of the rows and DIFFERS between consecutive calls — each case asserts both on the
eager twin — and a flag frozen at recording time shows in `lstm_state0` of the second replay.  Everything recorded takes device tensors
made before the recording (episode_start included: a NumPy array would be a host-to-device copy inside the capture).

  1  replay equals eager, per recurrent path         2  what a graph does not freeze (eager calls between replays)
  3  calls that refuse inside a capture               5  stream order, two handles on two streams / threads (eager, no graph)
"""
import ctypes as C
import threading

import numpy as np
import pytest

import policy_lstm_reference as L
from helpers import capture, gpu_batch
from policy_set_cases import COLUMNS, DEV, assert_columns_equal, close as _close, dev as _dev, env_sets, short_episodes, stagger, starts as _starts, stream as _stream
from reinforcement_learning_rendezvous_amd import _native as N
from test_gpu_graphs import Twin, _assert_same, _equal, _flat, _policy_states, _replay_equals_eager
from test_gpu_lstm_policy_sets import _member_weights, _set
from test_gpu_policy_lstm import _check_local, _noise_net, _policy, _state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T, REPLAYS, GAMMA, LAMBDA = 6, 3, 0.97, 0.9
SET_SIZES = (256, 256, 33)                      # 545 rows: no multiple of 4, three members, the tile table in use
GROUPED_SIZES = (256, 256)                      # test_gpu_lstm_policy_sets.py's grouped batch
ROLLOUT_COLUMNS = ("obs", "actions", "reward", "done", "log_prob", "last_obs")


def _nets(H, seed=0):
    """(actor, critic): a hot actor (the recursion matters) with the log_std of test_gpu_policy_lstm's noise network, a hot critic"""
    return dict(L.hot(H, seed=51 + seed), log_std=_noise_net(H)["log_std"]), L.critic_of(L.hot(H, seed=8 + seed))


def _short_env(n, seed=13):
    env = gpu_batch(n, params=short_episodes(), seed=seed)
    env.reset()
    stagger(env)
    return env


def _state_pair(n, H, seed=71):
    """a fixed device pair (h0, c0), |h| < 1"""
    rng = np.random.default_rng([seed, n, H])
    return _dev(rng.uniform(-0.9, 0.9, (n, H))), _dev(rng.uniform(-2.0, 2.0, (n, H)))


class _Made:
    """`make` of a case, keeping the twins it made: [0] graphed, [1] eager, in the order _replay_equals_eager makes them"""

    def __init__(self, build):
        self.build, self.twins = build, []

    def __call__(self):
        self.twins.append(self.build())
        return self.twins[-1]

    @property
    def eager(self):
        return self.twins[1]


def _note(t):
    """done[T-1] and lstm_state0 of the call just made, kept per twin for the preconditions (not inside a capture: a clone there is a node)"""
    if not torch.cuda.is_current_stream_capturing():
        t.__dict__.setdefault("last_done", []).append(t.out["done"][T - 1].clone())
        t.__dict__.setdefault("state0", []).append(tuple(x.clone() for x in t.out["lstm_state0"]))


def _rollout(t, deterministic=False):
    t.noise_counter(T)
    t.out = t.env.rollout(t.pol, T, deterministic=deterministic, out=t.out)
    _note(t)
    return t.out


def _collect(t):
    t.noise_counter(T)
    t.out = t.env.collect(t.pol, T, gamma=GAMMA, gae_lambda=LAMBDA, out=t.out)
    _note(t)
    return t.out


def _assert_flags_move(t, n):
    """The preconditions, on the eager twin's own outputs: the flags a call leaves pending are a strict, non-empty subset of the rows and
    differ from the next call's; `lstm_state0` of the call behind it is zero on exactly those rows.  A case that could not expose a stale
    flag fails here instead of passing silently."""
    torch.cuda.synchronize()
    assert len(t.last_done) >= 3
    for r, d in enumerate(t.last_done):
        assert 0 < int(d.sum()) < n, (r, int(d.sum()))
    for r, (a, b) in enumerate(zip(t.last_done, t.last_done[1:])):
        assert not torch.equal(a, b), f"done[T-1] of calls {r} and {r + 1} are equal: a stale flag would not show"
        h0 = t.state0[r + 1][0]
        zero = (h0 == 0).all(dim=1)
        assert torch.equal(zero, a.bool()), f"lstm_state0 of call {r + 1} is not zero on exactly the rows done at the end of call {r}"


# ------------------------------------------------------------------------------------------------------- 1: act, value, peek
@pytest.mark.parametrize("H", [32, 128])
def test_act_value_and_peek_replay_equal_eager(H):
    """Three steps in one graph over a fixed device tape of observations and flags, n = 300 (two 256-row workgroups, the second with a
    ragged last wave): a stochastic act with raw_out and log_prob_out, a committing value, a value(commit=False) on the next observation
    (it writes the scratch rows h_next and c_tmp only); then rdv_lstm_get_state of actor and critic inside the capture — and behind step
    0 as well, for the reference check.  Every output and both states after every replay, the outputs filled with NaN before it.

    The reference check: after the last replay the states of actor and critic are downloaded and the graph is replayed once more.  The
    first deterministic step of that replay is the critic's committing value of step 0: it and the critic's state behind it are held to
    the one-step float64 reference from the downloaded state (_check_local of test_gpu_policy_lstm.py, tolerance unchanged).  The actor's
    step 0 is stochastic, but its state is not: (h, c) behind it is held to the same one-step tolerance.  A replay that were wrong in
    the same way as its eager twin would still fail this."""
    n, steps = 300, 3
    actor, critic = _nets(H)
    obs_np = L.obs_sequence(n, steps + 1)
    flags_np = L.episode_starts(n, 4)[[2, 3, 1]]          # step 0: rows 0, 3, 6, ..; step 1: rows 1, 6, 11, ..; step 2: none
    assert 0 < int(flags_np[0].sum()) < n
    obs, flags = _dev(obs_np), _dev(flags_np, np.uint8)

    def build():
        pol = _policy(actor, critic, n, seed=9)
        b = dict(act=torch.empty((steps, n, 6), device=DEV), raw=torch.empty((steps, n, 6), device=DEV), lp=torch.empty((steps, n), device=DEV),
                 val=torch.empty((steps, n), device=DEV), peek=torch.empty((steps, n), device=DEV))
        return Twin(None, pol=pol, bufs=b)
    made = _Made(build)

    def fn(t):
        t.noise_counter(steps)
        b, states = t.bufs, {}
        for k in range(steps):
            t.pol.act(obs[k], episode_start=flags[k], deterministic=False, out=b["act"][k], raw_out=b["raw"][k], log_prob_out=b["lp"][k])
            t.pol.value(obs[k], episode_start=flags[k], out=b["val"][k])
            t.pol.value(obs[k + 1], commit=False, out=b["peek"][k])
            if k == 0:
                states["first"] = (t.pol.state, t.pol.critic_state)
        states["last"] = (t.pol.state, t.pol.critic_state)
        return b, states

    checked = []

    def reference_check(r, got, want):
        if r != REPLAYS - 1:
            return
        graphed, eager = made.twins
        before = {kind: _state(graphed.pol, kind) for kind in ("actor", "critic")}
        for _, x in _flat(got):
            x.fill_(float("nan"))
        graphed.graph.replay()
        again = fn(eager)                                     # the twins stay in step for the frame's final comparison
        torch.cuda.synchronize()
        _assert_same(got, again, "the reference replay")
        b, states = got
        a_after, c_after = ([x.cpu().numpy() for x in hc] for hc in states["first"])
        failures, worst = [], [0.0, 0.0, 0.0, ""]
        _check_local("replay", "critic", critic, obs_np[0], flags_np[0], before["critic"], b["val"][0].cpu().numpy().astype(np.float64)[:, None],
                     c_after, 0, worst, failures)
        assert not failures, failures
        bud = L.local_budget(actor, obs_np[0], flags_np[0], *before["actor"])
        for what, after in (("h", a_after[0]), ("c", a_after[1])):
            err, tol = float(np.abs(after.astype(np.float64) - bud[f"{what}64"]).max()), L.local_tolerance(bud, what)
            assert err <= tol, ("actor", what, err, tol)
        assert float(np.abs(before["actor"][0]).max()) > 0.01 and float(np.abs(before["critic"][1]).max()) > 0.01
        assert not any(torch.isnan(x).any() for _, x in _flat(got))
        checked.append(worst)
    _replay_equals_eager(made, fn, poison=True, after_replay=reference_check)
    assert len(checked) == 1


def test_state_calls_inside_the_capture():
    """[act, reset_state(r % 7 == 3), act, state = (h0, c0), act, reset_state(), act] recorded: rdv_lstm_reset_state (masked and whole),
    rdv_lstm_set_state and rdv_lstm_get_state as nodes of the graph; the four outputs and the state behind them after each replay."""
    n, H = 300, 32
    actor, critic = _nets(H)
    obs = _dev(L.obs_sequence(n, 4))
    mask = (torch.arange(n, device=DEV) % 7 == 3).to(torch.uint8)
    h0, c0 = _state_pair(n, H)

    def fn(t):
        t.noise_counter(4)
        p, out = t.pol, t.bufs
        p.act(obs[0], deterministic=False, out=out[0])
        p.reset_state(mask)
        p.act(obs[1], deterministic=False, out=out[1])
        masked = p.state
        p.state = (h0, c0)
        p.act(obs[2], deterministic=False, out=out[2])
        p.reset_state()
        p.act(obs[3], deterministic=False, out=out[3])
        return out, masked, p.state
    made = _Made(lambda: Twin(None, pol=_policy(actor, critic, n, seed=3), bufs=[torch.empty((n, 6), device=DEV) for _ in range(4)]))
    seen = {}
    _replay_equals_eager(made, fn, poison=True, after_replay=lambda r, got, want: seen.update(out=[x.clone() for x in want[0]]))
    a = seen["out"]
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[2], a[3]) and not torch.isnan(torch.stack(a)).any()


# ------------------------------------------------------------------------------------------------------- 1: rollout, collect
def _plain_case(n, H=32):
    actor, critic = _nets(H)
    return _Made(lambda: Twin(_short_env(n), pol=_policy(actor, critic, n, seed=9), out=None))


@pytest.mark.parametrize("n", [300, 33])
def test_rollout_replay_equals_eager(n):
    """rdv_rollout with an LstmPolicy, stochastic: every column, last_obs and lstm_state0 after each replay, at the end the actor's state
    and the env's state, bookkeeping and statistics.  n = 33: row t of [T, 33, 17] is not 16-byte aligned, the rows are copy nodes."""
    made = _plain_case(n)
    _replay_equals_eager(made, _rollout)
    _assert_flags_move(made.eager, n)


@pytest.mark.parametrize("n", [300, 33])
def test_collect_as_one_graph_equals_eager(n):
    """batch.collect with an LstmPolicy as ONE graph, `out` reused: the rollout's columns, values, last_value, advantages, returns and
    lstm_state0; at the end the actor's and the critic's state.  n = 33: the critic reads row t through obs_tmp.  n = 300 runs H = 128."""
    made = _plain_case(n, H=128 if n == 300 else 32)
    _replay_equals_eager(made, _collect)
    _assert_flags_move(made.eager, n)
    assert set(COLUMNS) <= set(made.eager.out)


def test_rollout_on_a_fresh_handle_starts_replay_0_from_the_warm_ups_flags():
    """The plain case, stated on its own so that a failure names it.  A handle is created with every row's start pending; the warm-up
    in helpers.capture consumes those flags (lstm_state0 of the first call is all zero) and leaves its own done[T-1] pending.  Replay 0
    starts from THOSE flags, as the eager twin's second call does: zero state on exactly the rows done at the end of the first call."""
    n = 300
    made = _plain_case(n)
    seen = {}
    _replay_equals_eager(made, _rollout, replays=1, after_replay=lambda r, got, want: seen.update(h=got["lstm_state0"][0].clone()))
    t = made.eager
    assert len(t.state0) == 2 and float(t.state0[0][0].abs().max()) == 0.0 and float(t.state0[0][1].abs().max()) == 0.0
    d = t.last_done[0].bool()
    assert 0 < int(d.sum()) < n
    assert torch.equal((seen["h"] == 0).all(dim=1), d), "replay 0 did not start from the warm-up's done[T-1]"


# ----------------------------------------------------------------------------------------------------------------- 1: sets
def _stagger_part(env, start):
    """policy_set_cases.stagger for rows [start, start + n) of a larger batch: the masks are those of the rows' GLOBAL indices"""
    n = env.num_envs
    zero = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    r = start + torch.arange(n, device=DEV)
    for s in range(4):
        env.step(zero)
        env.reset(mask=(r % 5 > s))


def _ungrouped_set_twin():
    return Twin(_short_env(sum(SET_SIZES), seed=12), pol=_set(64, SET_SIZES)[0], out=None)


def _grouped_set_twin():
    env = gpu_batch(sum(GROUPED_SIZES), params=env_sets()[:2], group_sizes=list(GROUPED_SIZES), seed=11)
    env.reset()
    stagger(env)
    return Twin(env, pol=_set(64, GROUPED_SIZES)[0], out=None)


def test_the_sets_eager_collect_equals_its_members():
    """The eager path the set replays below are compared with, tied once to the members: two collects of T = 6 of the set of (256, 256,
    33) on the ungrouped batch of 545 envs against three separate batches and stand-alone policies (policy_set_cases.assert_columns_equal,
    lstm_state0 included)."""
    t = _ungrouped_set_twin()
    _, members = _set(64, SET_SIZES)                             # the separate batches key the noise by their env_id_offset = start_g
    parts = [gpu_batch(m, params=short_episodes(), env_id_offset=s, seed=12) for s, m in zip(_starts(SET_SIZES), SET_SIZES)]
    for e, s in zip(parts, _starts(SET_SIZES)):
        e.reset()
        _stagger_part(e, s)
    for call in range(2):
        got = t.env.collect(t.pol, T, gamma=GAMMA, gae_lambda=LAMBDA)
        want = [e.collect(p, T, gamma=GAMMA, gae_lambda=LAMBDA) for e, p in zip(parts, members)]
        assert 0 < int(got["done"][T - 1].sum()) < sum(SET_SIZES)
        assert_columns_equal(got, want, f"call {call}", extra=("lstm_state0",))
    _close(t.env, t.pol, parts, members)


@pytest.mark.parametrize("which", ["ungrouped-545", "grouped"])
def test_set_collect_as_one_graph_equals_eager(which):
    """batch.collect with an LstmPolicySet as one graph: (256, 256, 33) on an ungrouped batch of 545 envs (545 % 4 = 1: the critic set
    reads its rows through obs_tmp), and (256, 256) on a grouped batch of policy_set_cases.env_sets (episodes of 6 and 8 steps: the
    second group's done[T-1] moves from call to call)."""
    made = _Made(_ungrouped_set_twin if which == "ungrouped-545" else _grouped_set_twin)
    _replay_equals_eager(made, _collect)
    _assert_flags_move(made.eager, made.eager.out["done"].shape[1])


# ------------------------------------------------------------------------------------------- 2: what a graph does not freeze
def test_eager_act_and_value_between_replays_of_a_collect():
    """An eager stochastic act and an eager committing value in front of replays 1 and 2, on the replaying stream: (h, c) of actor and
    critic move and the pending flags are cleared ON THE DEVICE.  The next replay's step 0, and its lstm_state0, use the cleared flags:
    no row of lstm_state0 is zero there, although done[T-1] of the replay before was not empty."""
    n = 300
    made = _plain_case(n)
    obs = _dev(L.obs_sequence(n, 2, seed=90))
    start = (torch.arange(n, device=DEV) % 3 == 0).to(torch.uint8)

    def eager_calls(t, r):
        if r in (1, 2):
            t.pol._calls = 100 + r
            t.pol.act(obs[r - 1], episode_start=start, deterministic=False)
            t.pol.value(obs[r - 1], episode_start=start)
    _replay_equals_eager(made, _collect, between=eager_calls, replays=4)
    t = made.eager                       # calls: 0 (the warm-up's), then replays 0..3
    torch.cuda.synchronize()
    for call in (2, 3):
        assert 0 < int(t.last_done[call - 1].sum()) < n
        assert not (t.state0[call][0] == 0).all(dim=1).any(), f"call {call}: a row of lstm_state0 is zero behind an eager act"
    assert torch.equal((t.state0[4][0] == 0).all(dim=1), t.last_done[3].bool())


def test_eager_set_state_and_reset_state_between_replays_of_a_rollout():
    """An eager pol.state = (h0, c0) and an eager reset_state(mask) in front of replays 1 and 2 of a recorded rollout: lstm_state0 of
    the replay behind them is (h0, c0) with the masked rows zero, no pending flag left."""
    n, H = 300, 32
    made = _plain_case(n, H)
    h0, c0 = _state_pair(n, H)
    mask = (torch.arange(n, device=DEV) % 7 == 3)

    def eager_calls(t, r):
        if r in (1, 2):
            t.pol.state = (h0, c0)
            t.pol.reset_state(mask.to(torch.uint8))
    _replay_equals_eager(made, _rollout, between=eager_calls, replays=4)
    t = made.eager
    torch.cuda.synchronize()
    keep, zero = (~mask)[:, None], torch.zeros((), device=DEV)
    for call in (2, 3):
        assert 0 < int(t.last_done[call - 1].sum()) < n
        assert _equal(t.state0[call][0], torch.where(keep, h0, zero)) and _equal(t.state0[call][1], torch.where(keep, c0, zero)), f"call {call}"


def _differs(a, b, names):
    return [k for k in names if not _equal(a[k], b[k])]


def test_eager_update_weights_between_replays_of_a_collect():
    """An eager update_weights(new) in front of replays 1 and 2 (two different dicts): the block is rewritten in the handle's existing
    allocation, so the graph stays valid and the replays behind it use the new weights.  A third twin that is never updated shows that
    they do: it equals replay 0 and differs from replay 1 on in actions, log_prob and values."""
    n, H = 300, 32
    made = _plain_case(n, H)
    new = {r: L.weights_dict(*_nets(H, seed=20 + r)) for r in (1, 2)}
    for r, w in new.items():
        w["log_std"] = w["log_std"] - np.float32(0.25 * r)        # log_prob depends on the noise and log_std alone
    third = made.build()
    _collect(third)
    _replay_equals_eager(made, _collect, between=lambda t, r: t.pol.update_weights(new[r]) if r in new else None, replays=4,
                         after_replay=lambda r, got, want: _third_twin(third, r, want))
    _assert_flags_move(made.eager, n)
    _close(third.env, third.pol)


def _third_twin(third, r, want):
    """the never-updated twin against the updated eager twin behind replay r: equal before the first update, different after it"""
    old = _collect(third)
    torch.cuda.synchronize()
    moved = _differs(old, want, ("actions", "log_prob", "values", "last_value"))
    if r == 0:
        assert not moved and not _differs(old, want, COLUMNS), moved
    else:
        assert moved == ["actions", "log_prob", "values", "last_value"], f"replay {r}: the new weights change nothing in {moved}"


def test_eager_refresh_of_one_member_between_replays_of_a_set_collect():
    """LstmPolicySet.update_weights(member=1, ...) in front of replays 1 and 2 of a recorded collect of the set of (256, 256, 33): member
    1's columns differ from a never-updated third twin's, the other members' columns still equal it."""
    made = _Made(_ungrouped_set_twin)
    new = {r: _member_weights(64, (64, 64), "tanh", 10 + r) for r in (1, 2)}
    third = made.build()
    _collect(third)
    sl = third.pol.group_slices

    def after(r, got, want):
        old = _collect(third)
        torch.cuda.synchronize()
        names = ("actions", "log_prob", "values")
        for g, s in enumerate(sl):
            moved = [k for k in names if not _equal(old[k][:, s].contiguous(), want[k][:, s].contiguous())]
            if r == 0 or g != 1:
                # the envs are independent: another member's rows see nothing of member 1's new weights
                assert not moved, f"replay {r}, member {g}: {moved} differ from the never-updated twin"
                for k in COLUMNS:
                    ax = (slice(None), s) if old[k].dim() > 1 and k != "last_obs" else (s,)
                    assert _equal(old[k][ax].contiguous(), want[k][ax].contiguous()), (r, g, k)
            else:
                assert moved == list(names), f"replay {r}: member 1's new weights change nothing in {set(names) - set(moved)}"
    _replay_equals_eager(made, _collect, between=lambda t, r: t.pol.update_weights(member=1, weights=new[r]) if r in new else None, replays=4,
                         after_replay=after)
    _assert_flags_move(made.eager, sum(SET_SIZES))
    _close(third.env, third.pol)


# ------------------------------------------------------------------------------------------------------------ 3: refusals
@pytest.mark.parametrize("call,on", [("rdv_lstm_set_weights", "plain"), ("rdv_lstm_set_member_weights", "set"), ("rdv_lstm_set_member_weights", "plain")])
def test_weight_refreshes_refuse_inside_a_capture(call, on):
    """[act, <call>, act] recorded, the call made through ctypes during the recording only: it returns RDV_ERR_INVALID_ARGUMENT with a
    message that starts with its name and says "stream capture" before it touches the stream; the capture ends normally, its replays
    are the two acts, and the same call succeeds eagerly afterwards."""
    lib = N.lib()
    H = 64
    n = sum(GROUPED_SIZES) if on == "set" else 300
    obs = _dev(L.obs_sequence(n, 2))

    def make():
        pol = _set(H, GROUPED_SIZES)[0] if on == "set" else _policy(*_nets(H), n, seed=4)
        return Twin(None, pol=pol, bufs=[torch.empty((n, 6), device=DEV) for _ in range(2)], refusal=None)
    graphed, eager = make(), make()
    source = graphed.pol[1] if on == "set" else graphed.pol              # the module whose arrays the call uploads: those the handle has
    lstm, ws, bs, log_std = source._host_arrays("l")
    args = (*[C.c_void_p(t.data_ptr()) for t in lstm], (C.c_void_p * len(ws))(*[t.data_ptr() for t in ws]),
            (C.c_void_p * len(bs))(*[t.data_ptr() for t in bs]), C.c_void_p(log_std[0].data_ptr()))

    def refresh(pol):
        h = pol._hip_handle(torch.device(DEV))
        if call == "rdv_lstm_set_weights":
            return lib.rdv_lstm_set_weights(h, *args, _stream())
        return lib.rdv_lstm_set_member_weights(h, 1 if on == "set" else 0, *args, _stream())

    def fn(t):
        t.noise_counter(2)
        t.pol.act(obs[0], deterministic=False, out=t.bufs[0])
        if t is graphed and torch.cuda.is_current_stream_capturing():
            rc = refresh(t.pol)
            t.refusal = (rc, lib.rdv_last_error().decode())
        t.pol.act(obs[1], deterministic=False, out=t.bufs[1])
        return t.bufs
    rec = {}
    g = capture(lambda: rec.update(out=fn(graphed)))          # ends normally: torch raises if the capture was invalidated
    rc, message = graphed.refusal
    assert rc == -1 and "stream capture" in message and message.startswith(call + ":"), (rc, message)
    fn(eager)
    for r in range(2):
        g.replay()
        want = fn(eager)
        torch.cuda.synchronize()
        _assert_same(rec["out"], want, f"replay {r}")
    assert refresh(graphed.pol) == 0, lib.rdv_last_error().decode()
    g.replay()                                                # the handle's own weights again: the graph is as valid as before
    want = fn(eager)
    torch.cuda.synchronize()
    _assert_same(rec["out"], want, "behind the eager refresh")
    _assert_same(_policy_states(graphed.pol), _policy_states(eager.pol), "final policy states")
    graphed.pol.close(); eager.pol.close()


# ------------------------------------------------------------------------------------------------------- 5: stream order
ORDER_ROWS = 65536                                                    # a kernel long enough to be running when the copy is enqueued


@pytest.mark.parametrize("middle", ["update_weights", "set_state"])
def test_recurrent_calls_are_ordered_on_the_callers_stream(middle):
    """act, update_weights(new) (or pol.state = (h0, c0)), act on a side stream with no synchronisation: the first output is the old
    network's on the state S0, the second the new network's on the state the first step left (or on (h0, c0)) — both equal a twin that
    ran the steps with a synchronise after every call; and the middle call matters: a policy that skips it gives another second output."""
    n, H = ORDER_ROWS, 32
    actor, critic = _nets(H)
    new = L.weights_dict(*_nets(H, seed=30))
    obs = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, size=(3, n, 17)).astype(np.float32)).to(DEV)
    rng = np.random.default_rng(2)
    h0, c0 = _dev(rng.uniform(-0.9, 0.9, (n, H))), _dev(rng.uniform(-2.0, 2.0, (n, H)))

    def mid(p):
        if middle == "update_weights":
            p.update_weights(new)
        else:
            p.state = (h0, c0)
    pol, twin, skip = (_policy(actor, critic, n) for _ in range(3))
    for p in (pol, twin, skip):
        p.act(obs[0], deterministic=True)                              # S0: not the zero state
    torch.cuda.synchronize()
    want = []
    for k, p in enumerate((twin, skip)):
        a = p.act(obs[1], deterministic=True).clone()
        torch.cuda.synchronize()
        if k == 0:
            mid(p)
            torch.cuda.synchronize()
        b = p.act(obs[2], deterministic=True).clone()
        torch.cuda.synchronize()
        want.append((a, b))
    assert _equal(want[0][0], want[1][0]) and not _equal(want[0][1], want[1][1])
    side = torch.cuda.Stream(device=DEV)
    a, b = torch.empty((n, 6), device=DEV), torch.empty((n, 6), device=DEV)
    with torch.cuda.stream(side):
        pol.act(obs[1], deterministic=True, out=a)
        mid(pol)
        pol.act(obs[2], deterministic=True, out=b)
        got_state = pol.state
    side.synchronize()
    assert _equal(a, want[0][0]) and _equal(b, want[0][1])
    for x, y in zip(got_state, twin.state):
        assert _equal(x, y)
    _close(pol, twin, skip)


PAIR_ENVS, PAIR_ROUNDS, PAIR_H = 1024, 4, 64


class LstmPair:
    """test_gpu_graphs.Pair with an LstmPolicy: an env batch and a recurrent policy of its own; `turns()` yields after every call of
    PAIR_ROUNDS x (rollout(T = 6), advantages)"""

    def __init__(self, seed):
        self.env = _short_env(PAIR_ENVS, seed=seed)
        self.pol = _policy(*_nets(PAIR_H, seed=seed), PAIR_ENVS, seed=seed + 100)
        dev = torch.device(DEV)
        self.pol._hip_handle(dev), self.pol._critic_handle(dev)
        self.rounds, self.out = [], None

    def turns(self):
        for _ in range(PAIR_ROUNDS):
            self.out = self.env.rollout(self.pol, T, out=self.out)
            yield
            self.pol.advantages(self.out, gamma=GAMMA, gae_lambda=LAMBDA)
            self.rounds.append({k: (self.out[k].clone() if k != "lstm_state0" else tuple(x.clone() for x in self.out[k])) for k in COLUMNS + ("lstm_state0",)})
            yield

    def result(self):
        return self.rounds, _policy_states(self.pol), self.env.get_state(), self.env.get_aux(), self.env.get_stats()

    def close(self):
        self.env.close(); self.pol.close()


@pytest.fixture(scope="module")
def solo_lstm_pairs():
    """each pair run alone on the default stream: the reference of both tests below (computed once, left unchanged)"""
    want = []
    for seed in (41, 42):
        p = LstmPair(seed)
        for _ in p.turns():
            pass
        torch.cuda.synchronize()
        want.append(p.result())
        p.close()
    assert not torch.equal(want[0][2], want[1][2]) and not torch.equal(want[0][1]["state"][0], want[1][1]["state"][0])
    assert 0 < int(want[0][0][-1]["done"][T - 1].sum()) < PAIR_ENVS
    return want


def _assert_lstm_pair(got, want, what):
    _assert_same(got[0], want[0], what)
    _assert_same(got[1], want[1], f"{what}: final policy states")
    assert _equal(got[2], want[2]) and _equal(got[3], want[3]) and got[4] == want[4], what


def test_two_lstm_pairs_on_two_streams_interleaved(solo_lstm_pairs):
    """one thread, two side streams, the two pairs' calls alternating one by one with no synchronisation in between: each handle's state,
    flags and scratch rows (h_next, c_tmp, obs_tmp) are its own"""
    pairs, streams = [LstmPair(41), LstmPair(42)], [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    turns = [p.turns() for p in pairs]
    for _ in range(2 * PAIR_ROUNDS):
        for s, it in zip(streams, turns):
            with torch.cuda.stream(s):
                next(it)
    got = []
    for s, p in zip(streams, pairs):
        with torch.cuda.stream(s):
            got.append(p.result())
    torch.cuda.synchronize()
    for k in range(2):
        _assert_lstm_pair(got[k], solo_lstm_pairs[k], f"pair {k}")
        pairs[k].close()


def test_two_lstm_pairs_from_two_threads(solo_lstm_pairs):
    """different handles from different threads (include/rdv.h): ctypes releases the GIL around every call, the two pairs' launches run
    concurrently"""
    pairs, streams = [LstmPair(41), LstmPair(42)], [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, failures = [None, None], []
    start = threading.Barrier(2)

    def work(k):
        try:
            start.wait(timeout=60)
            with torch.cuda.stream(streams[k]):
                for _ in pairs[k].turns():
                    pass
                got[k] = pairs[k].result()
            streams[k].synchronize()
        except BaseException as exc:        # reported by the main thread
            failures.append((k, exc))
            start.abort()
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not failures, failures
    assert not any(t.is_alive() for t in threads)
    torch.cuda.synchronize()
    for k in range(2):
        _assert_lstm_pair(got[k], solo_lstm_pairs[k], f"pair {k}")
        pairs[k].close()

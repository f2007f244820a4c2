"""
GPU: rdv_ppo_mlp_set_loss_grad (include/rdv.h, "PPO minibatch gradients for policy sets of every MLP architecture"; csrc/rdv_ppo_mlp.h,
"the set form") and PolicySet.ppo_grads of sets of other architectures than the shipped one, held to their specification by EQUALITY:

    every output of member g is bit for bit what rdv_ppo_mlp_loss_grad writes for stand-alone handles of member g's weights and the
    set's two specs, given the same rows, indices + off_g, n = counts[g] and the same coefficients.

rdv_ppo_mlp_loss_grad itself is held to the fp64 reference by tests/test_gpu_ppo_mlp_grad.py, so no tolerance appears here.  Spec pairs
and members: tests/ppo_mlp_set_helpers.py.  Counts: a lone lane, both sides of a wave's 32 rows and of a workgroup's 128 and 256 rows,
more than one workgroup, an idle workgroup column, skipped members; pair (b)'s actor cuts a member's rows into 128-row workgroups and its
critic into 256-row ones, so the two nets' grids differ.  Outputs are compared as bit patterns (int32 views).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_reference as M
import ppo_mlp_set_helpers as H
import ppo_reference as P
import test_ppo_set_grad as S
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd import ppo
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy, PolicySet
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy, LstmPolicySet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENT, VF = 0.01, 0.5
NAN = float("nan")
CASES = [("a", (33, 0, 257)), ("a", (1, 549, 32)), ("b", (129, 1, 0)), ("b", (127, 257, 128)), ("c", (129, 0, 33)), ("d", (1, 0, 0)),
         ("d", (256, 31, 1))]


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_WORLDS = {}


def world(key):
    """(set, stand-alone policies of the members' weights, device columns) of one pair; made once, left unchanged."""
    if key not in _WORLDS:
        pair = H.PAIRS[key]
        cols = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in H.columns(pair).items()}
        _WORLDS[key] = (H.make_set(pair).to(DEV), [H.policy_of(n).to(DEV) for n in H.member_nets(pair)], cols)
    return _WORLDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for pset, alone, _ in _WORLDS.values():
        pset.close()
        for p in alone:
            p.close()
    _WORLDS.clear()


def index_vectors(counts):
    return [torch.as_tensor(P.index_vector(n, seed=9 + g), device=DEV) if n else None for g, n in enumerate(counts)]


def grad_floats(sa, sc):
    return int(N.lib().rdv_ppo_mlp_grad_floats(C.byref(sa), 1)), int(N.lib().rdv_ppo_mlp_grad_floats(C.byref(sc), 0))


def alone_call(pol, pair, cols, idx, eps=P.EPS):
    """rdv_ppo_mlp_loss_grad on stand-alone handles -> (actor_grad, critic_grad, scalars, log_prob, values)"""
    lib, n = N.lib(), int(idx.numel())
    sa, sc = H.specs(pair)
    ws = torch.full((int(lib.rdv_ppo_mlp_workspace_bytes(C.byref(sa), C.byref(sc), n)) // 4,), NAN, device=DEV)
    outs = [torch.full((k,), NAN, device=DEV) for k in (*grad_floats(sa, sc), N.PPO_SCALARS, n, n)]
    rows = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["old_log_prob"].data_ptr(), cols["advantages"].data_ptr(),
                     cols["returns"].data_ptr(), idx.data_ptr(), cols["obs"].shape[0])
    out = N.PpoOut(*[t.data_ptr() for t in outs])
    N.check(lib.rdv_ppo_mlp_loss_grad(pol._hip_handle(DEV), pol._critic_handle(DEV), C.byref(rows), n, eps, ENT, VF, C.c_void_p(ws.data_ptr()),
                                      ws.numel() * 4, C.byref(out), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    return outs


class SetCall:
    """The arguments of one rdv_ppo_mlp_set_loss_grad: outputs and workspace pre-filled with NaN; ``run`` enqueues on the current stream."""

    def __init__(self, pair, cols, counts, idx, workspace_bytes=None, null_indices=False):
        lib = N.lib()
        self.P = len(counts)
        self.counts = (C.c_int64 * len(counts))(*counts)
        total = sum(counts)
        self.idx = torch.cat([i for i in idx if i is not None])
        assert self.idx.numel() == total
        sa, sc = H.specs(pair)
        need = int(lib.rdv_ppo_mlp_set_workspace_bytes(C.byref(sa), C.byref(sc), len(counts), self.counts))
        assert need > 0
        self.ws = torch.full(((need if workspace_bytes is None else workspace_bytes) // 4,), NAN, device=DEV)
        ga, gc = grad_floats(sa, sc)
        self.outs = [torch.full(s, NAN, device=DEV) for s in ((self.P, ga), (self.P, gc), (self.P, N.PPO_SCALARS), (total,), (total,))]
        self.rows = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["old_log_prob"].data_ptr(), cols["advantages"].data_ptr(),
                              cols["returns"].data_ptr(), None if null_indices else self.idx.data_ptr(), cols["obs"].shape[0])
        self.out = N.PpoSetOut(*[t.data_ptr() for t in self.outs])

    def run(self, actor, critic, eps=P.EPS, fn="rdv_ppo_mlp_set_loss_grad"):
        return getattr(N.lib(), fn)(actor, critic, C.byref(self.rows), self.counts, eps, ENT, VF, C.c_void_p(self.ws.data_ptr()), self.ws.numel() * 4,
                                    C.byref(self.out), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def set_call(pset, pair, cols, counts, idx):
    c = SetCall(pair, cols, counts, idx)
    N.check(c.run(pset._hip_handle(DEV), pset._critic_handle(DEV)))
    torch.cuda.synchronize()
    return c.outs


def assert_members_equal_alone(outs, alone, pair, cols, counts, idx):
    off = 0
    for g, n in enumerate(counts):
        if n == 0:
            assert all(bool(torch.isnan(t[g]).all()) for t in outs[:3]), g      # nothing of a skipped member is written
            continue
        ref = alone_call(alone[g], pair, cols, idx[g])
        for name, got, want in zip(("actor_grad", "critic_grad", "scalars"), outs[:3], ref[:3]):
            assert bits_equal(got[g], want), (g, name)
            assert bool(torch.isfinite(want[:6]).all())
        assert bool((ref[1] != 0).any())
        assert bits_equal(outs[3][off:off + n], ref[3]), (g, "log_prob")
        assert bits_equal(outs[4][off:off + n], ref[4]), (g, "values")
        off += n
    assert off == outs[3].numel()


@pytest.mark.parametrize("key,counts", CASES, ids=[k + "-" + "-".join(map(str, c)) for k, c in CASES])
def test_every_member_gets_the_bits_of_the_stand_alone_call(key, counts):
    pset, alone, cols = world(key)
    pair = H.PAIRS[key]
    assert ppo.hip_set_route(pset) == "mlp"
    idx = index_vectors(counts)
    for i in idx:
        if i is not None and i.numel() >= 4:
            assert len(set(i.tolist())) < i.numel()                 # shuffled, some rows repeated
    outs = set_call(pset, pair, cols, counts, idx)
    assert_members_equal_alone(outs, alone, pair, cols, counts, idx)
    live = [g for g, n in enumerate(counts) if n]
    if len(live) > 1:                                               # a wrong member's block cannot pass: the members' gradients differ
        assert not bits_equal(outs[1][live[0]], outs[1][live[1]])


def test_sixty_four_members_a_third_of_them_sitting_out():
    """The by-value table at its limit: P = 64 members of [16] sigmoid, counts[g] = g % 3; the rows of the members that sit out keep
    their sentinel."""
    pair = ((16,), (16,), "sigmoid")
    nets = H.member_nets(pair, 64)
    sizes = [256] * 63 + [P.ROWS]
    pset = PolicySet([H.policy_of(n) for n in nets], sizes).to(DEV)
    cols = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in H.columns(pair).items()}
    counts = tuple(g % 3 for g in range(64))
    idx = [torch.as_tensor(P.index_vector(n, seed=9 + g), device=DEV) if n else None for g, n in enumerate(counts)]
    try:
        outs = set_call(pset, pair, cols, counts, idx)
        for g in (1, 2, 31, 62):                                    # stand-alone handles of a few members: both counts, both ends
            alone = H.policy_of(nets[g]).to(DEV)
            ref = alone_call(alone, pair, cols, idx[g])
            off = sum(counts[:g])
            for got, want in zip((outs[0][g], outs[1][g], outs[2][g], outs[3][off:off + counts[g]], outs[4][off:off + counts[g]]), ref):
                assert bits_equal(got, want), g
            alone.close()
        for g, n in enumerate(counts):
            written = [not bool(torch.isnan(t[g]).any()) for t in outs[:3]]
            assert written == [n > 0] * 3, g
            if n == 0:
                assert all(bool(torch.isnan(t[g]).all()) for t in outs[:3]), g
    finally:
        pset.close()


def test_two_eager_calls_and_a_graph_replay_give_the_same_bits():
    pset, alone, cols = world("b")
    pair, counts = H.PAIRS["b"], (127, 257, 128)
    idx = index_vectors(counts)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
    results = []
    for _ in range(2):
        call = SetCall(pair, cols, counts, idx)
        N.check(call.run(a, c))
        torch.cuda.synchronize()
        results.append([t.clone() for t in call.outs])
    call = SetCall(pair, cols, counts, idx)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        N.check(call.run(a, c))                                     # (the LDS limits are raised outside the capture)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            N.check(call.run(a, c))
        for t in call.outs:
            t.fill_(NAN)
        call.ws.fill_(NAN)
        g.replay()
        stream.synchronize()
    results.append(call.outs)
    for other in results[1:]:
        for x, y in zip(results[0], other):
            assert bits_equal(x, y)
    assert all(bool(torch.isfinite(t).all()) for t in results[0])
    assert_members_equal_alone(results[2], alone, pair, cols, counts, idx)      # the replayed outputs, against the stand-alone call


def test_a_call_behind_set_member_weights_differentiates_that_members_new_block():
    _, alone, cols = world("a")
    pair, counts = H.PAIRS["a"], (33, 257, 31)
    idx = index_vectors(counts)
    new = H.member_nets(pair, 8)[7]
    pset = H.make_set(pair).to(DEV)
    fresh = H.policy_of(new).to(DEV)
    try:
        before = set_call(pset, pair, cols, counts, idx)            # the handles exist and hold the old weights
        pset.update_weights(member=1, weights=M.weights_dict(*new))  # rdv_policy_set_member_weights on the current stream
        after = set_call(pset, pair, cols, counts, idx)
        assert_members_equal_alone(after, [alone[0], fresh, alone[2]], pair, cols, counts, idx)
        for t0, t1 in zip(before[:3], after[:3]):
            assert bits_equal(t0[0], t1[0]) and bits_equal(t0[2], t1[2]) and not bits_equal(t0[1], t1[1])
    finally:
        pset.close(); fresh.close()


def test_default_spec_sets_get_the_bits_of_the_shipped_set_call():
    pair = ((64, 64), (64, 64), "tanh")
    counts = (33, 0, 257)
    idx = index_vectors(counts)
    pset = S.make_set().to(DEV)
    cols = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in S.set_columns().items()}
    try:
        a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
        assert ppo.hip_set_route(pset) == "shipped"
        got, want = SetCall(pair, cols, counts, idx), SetCall(pair, cols, counts, idx)
        N.check(got.run(a, c))
        N.check(want.run(a, c, fn="rdv_ppo_set_loss_grad"))
        torch.cuda.synchronize()
        for x, y in zip(got.outs, want.outs):
            assert bits_equal(x, y)
        assert bool(torch.isfinite(got.outs[0][0]).all()) and bool(torch.isnan(got.outs[0][1]).all())
        # its refusals are the shipped call's
        short = SetCall(pair, cols, counts, idx, workspace_bytes=64)
        assert short.run(a, c) == -1 and "rdv_ppo_set_loss_grad: workspace_bytes" in N.lib().rdv_last_error().decode()
    finally:
        pset.close()


def test_a_set_of_one_member_and_a_plain_handle_pair_are_accepted():
    _, alone, cols = world("a")
    pair = H.PAIRS["a"]
    idx = index_vectors((549,))
    ref = alone_call(alone[1], pair, cols, idx[0])
    single = PolicySet([alone[1]], [P.ROWS])
    try:
        for actor, critic in ((single._hip_handle(DEV), single._critic_handle(DEV)), (alone[1]._hip_handle(DEV), alone[1]._critic_handle(DEV))):
            assert N.lib().rdv_policy_num_members(actor) == 1
            call = SetCall(pair, cols, (549,), idx)
            N.check(call.run(actor, critic))
            torch.cuda.synchronize()
            for got, want in zip(call.outs, ref):
                assert bits_equal(got.reshape(-1), want)
    finally:
        single.close()


def test_refusals_enqueue_nothing_and_leave_the_handles_usable():
    pset, alone, cols = world("a")
    pair, counts = H.PAIRS["a"], (33, 0, 257)
    idx = index_vectors(counts)
    before = set_call(pset, pair, cols, counts, idx)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
    shipped = S.make_set()
    two = PolicySet([alone[0], alone[1]], [256, 944])
    lstm = LstmPolicy(lstm_hidden_size=32, net_arch=[64, 64], n_rows=64)
    lset = LstmPolicySet([LstmPolicy(lstm_hidden_size=32, net_arch=[64, 64]) for _ in range(3)], H.SIZES)
    try:
        for kw, handles, words in ((dict(), (shipped._hip_handle(DEV), c), ("actor_set has the default spec", "mixed pair")),
                                   (dict(), (a, shipped._critic_handle(DEV)), ("critic_set has the default spec", "mixed pair")),
                                   (dict(), (lstm._hip_handle(DEV), c), ("actor_set", "recurrent")),
                                   (dict(), (a, lset._critic_handle(DEV)), ("critic_set", "recurrent")),
                                   (dict(), (c, a), ("swapped",)),
                                   (dict(), (a, two._critic_handle(DEV)), ("actor_set has 3 members", "critic_set has 2")),
                                   (dict(workspace_bytes=64), (a, c), ("workspace_bytes", "rdv_ppo_mlp_set_workspace_bytes")),
                                   (dict(null_indices=True), (a, c), ("rows->indices is null",))):
            call = SetCall(pair, cols, counts, idx, **kw)
            rc = call.run(*handles)
            msg = N.lib().rdv_last_error().decode()
            assert rc == -1 and all(w in msg for w in words) and "rdv_ppo_mlp_set_loss_grad" in msg, (words, rc, msg)
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in call.outs)       # a refused call enqueues nothing
        after = set_call(pset, pair, cols, counts, idx)
        for x, y in zip(before, after):
            assert bits_equal(x, y)
    finally:
        for p in (shipped, two, lstm, lset):
            p.close()


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "raw"])
def test_ppo_grads_equals_ppo_grad_of_each_member_alone(normalize):
    pair = H.PAIRS["a"]
    _, _, cols = world("a")
    buf = H.make_buf(cols)
    pset = H.make_set(pair).to(DEV)
    alone = [H.policy_of(n).to(DEV) for n in H.member_nets(pair)]
    try:
        assert ppo.hip_set_route(pset) == "mlp"
        for counts in ((33, 0, 257), (256, 31, 1)):
            idx = [H.member_indices(g, n).to(DEV) if n else None for g, n in enumerate(counts)]
            kept = [p.grad.clone() if p.grad is not None else None for p in pset[1].parameters()]
            out = pset.ppo_grads(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)
            assert tuple(pset._ppo[torch.device(DEV)]["actor"].shape) == (3, sum(p.numel() for p in ppo._params(pset[0])[0]))
            for g, n in enumerate(counts):
                if n == 0:
                    assert out[g] is None
                    assert all((p.grad is None and k is None) or bits_equal(p.grad, k) for p, k in zip(pset[g].parameters(), kept))
                    continue
                s = alone[g].ppo_grad(buf, idx[g], clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)
                for (name, x), y in zip(pset[g].named_parameters(), alone[g].parameters()):
                    assert bits_equal(x.grad, y.grad), (counts, g, name)
                assert any(bool((p.grad != 0).any()) for p in pset[g].parameters())
                assert set(out[g]) == set(s) and all(out[g][k].dim() == 0 and bits_equal(out[g][k], s[k]) for k in s)
    finally:
        pset.close()
        for p in alone:
            p.close()

"""
GPU: rdv_ppo_set_loss_grad (include/rdv.h, "PPO minibatch gradients for policy sets"; csrc/rdv_ppo.h, "the set form") and
PolicySet.ppo_grads, held to their specification by EQUALITY:

    every output of member g is bit for bit what rdv_ppo_loss_grad writes for stand-alone handles of member g's weights, given the same
    rows, indices + off_g, n = counts[g] and the same coefficients.

rdv_ppo_loss_grad itself is held to the fp64 reference by tests/test_gpu_ppo_grad.py, so no tolerance appears here.  The set, the members
and the columns are those of tests/test_ppo_set_grad.py: sizes [256, 512, 432] over 1,200 rows seen as T = 1, N = 1200; the golden
checkpoint, the dense random member and a third dense member.  Count vectors (33, 0, 257), (1, 549, 32), (256, 31, 1): a lone lane, both
sides of a wave's 32-row tile and of a workgroup's 256 rows, three workgroups whose last wave is partly filled, an idle workgroup column
(the grid is as wide as the largest member needs), a skipped member.  Outputs are compared as bit patterns (int32 views).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_reference as M
import ppo_reference as P
import test_ppo_set_grad as S
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy, PolicySet
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicy, LstmPolicySet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENT, VF = 0.01, 0.5
COUNTS = [(33, 0, 257), (1, 549, 32), (256, 31, 1)]
NAN = float("nan")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def policy_of(nets):
    return MlpPolicy(M.weights_dict(*nets)).to(DEV)


@pytest.fixture(scope="module")
def world():
    """The set, three stand-alone policies of the members' weights, the columns on the device; made once, left unchanged."""
    pset = S.make_set().to(DEV)
    alone = [policy_of(n) for n in S.member_nets()]
    cols = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in S.set_columns().items()}
    yield pset, alone, cols
    pset.close()
    for p in alone:
        p.close()


def index_vectors(counts):
    """Per member a shuffled index vector with duplicates that reaches rows 0 and 1199 (ppo_reference.index_vector), another per member"""
    return [torch.as_tensor(P.index_vector(n, seed=9 + g), device=DEV) if n else None for g, n in enumerate(counts)]


def alone_call(pol, cols, idx, eps=P.EPS):
    """rdv_ppo_loss_grad on stand-alone handles -> (actor_grad, critic_grad, scalars, log_prob, values)"""
    lib, n = N.lib(), int(idx.numel())
    ws = torch.full((int(lib.rdv_ppo_workspace_bytes(n)) // 4,), NAN, device=DEV)
    outs = [torch.full((k,), NAN, device=DEV) for k in (N.PPO_ACTOR_GRAD, N.PPO_CRITIC_GRAD, N.PPO_SCALARS, n, n)]
    rows = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["old_log_prob"].data_ptr(), cols["advantages"].data_ptr(),
                     cols["returns"].data_ptr(), idx.data_ptr(), cols["obs"].shape[0])
    out = N.PpoOut(*[t.data_ptr() for t in outs])
    N.check(lib.rdv_ppo_loss_grad(pol._hip_handle(DEV), pol._critic_handle(DEV), C.byref(rows), n, eps, ENT, VF, C.c_void_p(ws.data_ptr()),
                                  ws.numel() * 4, C.byref(out), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    return outs


class SetCall:
    """The arguments of one rdv_ppo_set_loss_grad: outputs and workspace pre-filled with NaN; ``run`` enqueues on the current stream."""

    def __init__(self, cols, counts, idx, workspace_bytes=None, null_indices=False):
        lib = N.lib()
        self.P = len(counts)
        self.counts = (C.c_int64 * len(counts))(*counts)
        total = sum(counts)
        self.idx = torch.cat([i for i in idx if i is not None])
        assert self.idx.numel() == total
        need = int(lib.rdv_ppo_set_workspace_bytes(len(counts), self.counts))
        self.ws = torch.full(((need if workspace_bytes is None else workspace_bytes) // 4,), NAN, device=DEV)
        self.outs = [torch.full(s, NAN, device=DEV) for s in ((self.P, N.PPO_ACTOR_GRAD), (self.P, N.PPO_CRITIC_GRAD), (self.P, N.PPO_SCALARS), (total,), (total,))]
        self.rows = N.PpoRows(cols["obs"].data_ptr(), cols["actions"].data_ptr(), cols["old_log_prob"].data_ptr(), cols["advantages"].data_ptr(),
                              cols["returns"].data_ptr(), None if null_indices else self.idx.data_ptr(), cols["obs"].shape[0])
        self.out = N.PpoSetOut(*[t.data_ptr() for t in self.outs])

    def run(self, actor, critic, eps=P.EPS):
        return N.lib().rdv_ppo_set_loss_grad(actor, critic, C.byref(self.rows), self.counts, eps, ENT, VF, C.c_void_p(self.ws.data_ptr()), self.ws.numel() * 4,
                                             C.byref(self.out), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def set_call(pset, cols, counts, idx):
    c = SetCall(cols, counts, idx)
    N.check(c.run(pset._hip_handle(DEV), pset._critic_handle(DEV)))
    torch.cuda.synchronize()
    return c.outs


def assert_members_equal_alone(outs, alone, cols, counts, idx):
    off = 0
    for g, n in enumerate(counts):
        if n == 0:
            assert all(bool(torch.isnan(t[g]).all()) for t in outs[:3]), g      # nothing of a skipped member is written
            continue
        ref = alone_call(alone[g], cols, idx[g])
        for name, got, want in zip(("actor_grad", "critic_grad", "scalars"), outs[:3], ref[:3]):
            assert bits_equal(got[g], want), (g, name)
            assert bool(torch.isfinite(want[:6]).all())
        assert bool((ref[0] != 0).any()) and bool((ref[1] != 0).any())
        assert bits_equal(outs[3][off:off + n], ref[3]), (g, "log_prob")
        assert bits_equal(outs[4][off:off + n], ref[4]), (g, "values")
        off += n
    assert off == outs[3].numel()


@pytest.mark.parametrize("counts", COUNTS, ids=["-".join(map(str, c)) for c in COUNTS])
def test_every_member_gets_the_bits_of_the_stand_alone_call(world, counts):
    pset, alone, cols = world
    idx = index_vectors(counts)
    for i in idx:
        if i is not None and i.numel() >= 4:
            assert int(i.min()) == 0 and int(i.max()) == P.ROWS - 1 and len(set(i.tolist())) < i.numel()
    outs = set_call(pset, cols, counts, idx)
    assert_members_equal_alone(outs, alone, cols, counts, idx)
    # a wrong member's block cannot pass: the members' gradients differ from one another
    live = [g for g, n in enumerate(counts) if n]
    assert not bits_equal(outs[0][live[0]], outs[0][live[1]]) and not bits_equal(outs[1][live[0]], outs[1][live[1]])


def test_a_member_of_256_workgroups_gets_the_bits_of_the_stand_alone_call(world):
    """Counts (65536, 0, 300): a member whose rows fill 256 workgroups beside a skipped one and one of two workgroups — the sum over
    workgroups of the shared finishing body at the size the stand-alone call is pinned at (tests/test_gpu_ppo_grad.py).  The index
    vectors draw from the 1,200 rows with repetition."""
    pset, alone, cols = world
    counts = (65536, 0, 300)
    rng = np.random.default_rng(21)
    idx = [torch.as_tensor(rng.integers(0, P.ROWS, size=n), device=DEV) if n else None for n in counts]
    outs = set_call(pset, cols, counts, idx)
    assert_members_equal_alone(outs, alone, cols, counts, idx)
    assert not bits_equal(outs[0][0], outs[0][2]) and not bits_equal(outs[1][0], outs[1][2])


def test_two_eager_calls_and_a_graph_replay_give_the_same_bits(world):
    pset, _, cols = world
    counts = (1, 549, 32)
    idx = index_vectors(counts)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
    results = []
    for _ in range(2):
        call = SetCall(cols, counts, idx)
        N.check(call.run(a, c))
        torch.cuda.synchronize()
        results.append([t.clone() for t in call.outs])
    call = SetCall(cols, counts, idx)
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


def test_a_call_behind_set_member_weights_differentiates_that_members_new_block(world):
    _, alone, cols = world
    counts = (33, 257, 31)
    idx = index_vectors(counts)
    new = P.random_nets(seed=41)
    pset = S.make_set().to(DEV)
    fresh = policy_of(new)
    try:
        before = set_call(pset, cols, counts, idx)                  # the handles exist and hold the old weights
        pset.update_weights(member=1, weights=M.weights_dict(*new))  # rdv_policy_set_member_weights on the current stream
        after = set_call(pset, cols, counts, idx)
        assert_members_equal_alone(after, [alone[0], fresh, alone[2]], cols, counts, idx)
        for t0, t1 in zip(before[:3], after[:3]):
            assert bits_equal(t0[0], t1[0]) and bits_equal(t0[2], t1[2]) and not bits_equal(t0[1], t1[1])
    finally:
        pset.close(); fresh.close()


def test_refusals_leave_the_handles_usable(world):
    pset, alone, cols = world
    counts = COUNTS[0]
    idx = index_vectors(counts)
    before = set_call(pset, cols, counts, idx)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
    wide_nets = (M.dense([32, 32], "tanh"), M.critic_of(M.dense([32, 32], "tanh")))
    wide = PolicySet([MlpPolicy(M.weights_dict(*wide_nets)) for _ in range(3)], S.SIZES)
    two = PolicySet([alone[0], alone[1]], [256, 944])
    lstm = LstmPolicy(lstm_hidden_size=32, net_arch=[64, 64], n_rows=64)
    lset = LstmPolicySet([LstmPolicy(lstm_hidden_size=32, net_arch=[64, 64]) for _ in range(3)], S.SIZES)
    try:
        for kw, handles, words in ((dict(), (lstm._hip_handle(DEV), c), ("actor_set", "recurrent")),
                                   (dict(), (a, lset._critic_handle(DEV)), ("critic_set", "recurrent")),
                                   (dict(), (c, a), ("swapped",)),
                                   (dict(), (wide._hip_handle(DEV), c), ("actor_set", "shipped architecture")),
                                   (dict(), (a, wide._critic_handle(DEV)), ("critic_set", "shipped architecture")),
                                   (dict(), (a, two._critic_handle(DEV)), ("actor_set has 3 members", "critic_set has 2")),
                                   (dict(workspace_bytes=64), (a, c), ("workspace_bytes",)),
                                   (dict(null_indices=True), (a, c), ("rows->indices is null",))):
            call = SetCall(cols, counts, idx, **kw)
            rc = call.run(*handles)
            msg = N.lib().rdv_last_error().decode()
            assert rc == -1 and all(w in msg for w in words) and "rdv_ppo_set_loss_grad" in msg, (words, rc, msg)
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in call.outs)       # a refused call enqueues nothing
        # the stand-alone call still refuses a set by name
        n = 33
        ws = torch.empty(int(N.lib().rdv_ppo_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        one = SetCall(cols, (n,), [idx[0]])
        out = N.PpoOut(*[t.data_ptr() for t in one.outs])
        rc = N.lib().rdv_ppo_loss_grad(a, c, C.byref(one.rows), n, P.EPS, ENT, VF, C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(out), None)
        assert rc == -1 and "policy set" in N.lib().rdv_last_error().decode()
        after = set_call(pset, cols, counts, idx)
        for x, y in zip(before, after):
            assert bits_equal(x, y)
        assert_members_equal_alone(after, alone, cols, counts, idx)
    finally:
        for p in (wide, two, lstm, lset):
            p.close()


def test_a_set_of_one_member_and_a_plain_handle_pair_are_accepted(world):
    _, alone, cols = world
    idx = index_vectors((549,))
    ref = alone_call(alone[1], cols, idx[0])
    single = PolicySet([alone[1]], [P.ROWS])
    try:
        for actor, critic in ((single._hip_handle(DEV), single._critic_handle(DEV)), (alone[1]._hip_handle(DEV), alone[1]._critic_handle(DEV))):
            assert N.lib().rdv_policy_num_members(actor) == 1
            call = SetCall(cols, (549,), idx)
            N.check(call.run(actor, critic))
            torch.cuda.synchronize()
            for got, want in zip(call.outs, ref):
                assert bits_equal(got.reshape(-1), want)
    finally:
        single.close()


def _buf(cols):
    return {("log_prob" if k == "old_log_prob" else k): v.reshape(1, P.ROWS, *v.shape[1:]) for k, v in cols.items()}


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "raw"])
def test_ppo_grads_equals_ppo_grad_of_each_member_alone(world, normalize):
    _, _, cols = world
    buf = _buf(cols)
    pset = S.make_set().to(DEV)
    alone = [policy_of(n) for n in S.member_nets()]
    try:
        for counts in ((33, 0, 257), (256, 31, 1)):
            idx = [S.member_indices(g, n).to(DEV) if n else None for g, n in enumerate(counts)]
            kept = [p.grad.clone() if p.grad is not None else None for p in pset[1].parameters()]
            out = pset.ppo_grads(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)
            for g, n in enumerate(counts):
                if n == 0:
                    assert out[g] is None
                    assert all((p.grad is None and k is None) or bits_equal(p.grad, k) for p, k in zip(pset[g].parameters(), kept))
                    continue
                s = alone[g].ppo_grad(buf, idx[g], clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)
                for (name, a), b in zip(pset[g].named_parameters(), alone[g].parameters()):
                    assert bits_equal(a.grad, b.grad) and bool((a.grad != 0).any()), (counts, g, name)
                assert set(out[g]) == set(s) and all(out[g][k].dim() == 0 and bits_equal(out[g][k], s[k]) for k in s)
    finally:
        pset.close()
        for p in alone:
            p.close()


def test_three_update_steps_of_the_set_equal_three_stand_alone_learners(world):
    """The loop of INTEGRATION.md, three steps: ppo_grads, clip_grad_norm_ per member, ONE Adam over all members' parameters,
    update_weights — against three stand-alone copies with the same minibatches (ppo_grad, clip_grad_norm_, an Adam each, update_weights).
    Adam is element-wise, so one optimiser over all members takes the steps of three."""
    _, _, cols = world
    buf = _buf(cols)
    pset = S.make_set().to(DEV)
    alone = [policy_of(n) for n in S.member_nets()]
    try:
        opt = torch.optim.Adam([p for member in pset for p in member.parameters()], lr=3e-4)
        opts = [torch.optim.Adam(pol.parameters(), lr=3e-4) for pol in alone]
        obs = cols["obs"]
        pset.act(obs); pset.value(obs)                              # the handles exist before the first update_weights
        steps = [(200, 200, 200), (56, 200, 200), (0, 112, 32)]      # the last pieces of an epoch run out unequally
        for counts in steps:
            idx = [S.member_indices(g, n, seed=counts[1]).to(DEV) if n else None for g, n in enumerate(counts)]
            pset.ppo_grads(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
            for g, member in enumerate(pset):
                if idx[g] is not None:
                    torch.nn.utils.clip_grad_norm_(member.parameters(), 0.5)
                else:                                               # a member that sits the step out takes no optimiser step either
                    for p in member.parameters():
                        p.grad = None
            opt.step()
            pset.update_weights()
            for g, pol in enumerate(alone):
                if idx[g] is not None:
                    pol.ppo_grad(buf, idx[g], clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
                    torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
                    opts[g].step()
                    pol.update_weights()
        for g in range(3):
            for (name, a), b in zip(pset[g].named_parameters(), alone[g].parameters()):
                assert torch.equal(a, b), (g, name)
        got, values = pset.act(obs), pset.value(obs)
        for g, sl in enumerate(pset.group_slices):
            assert torch.equal(got[sl], alone[g].act(obs[sl]))
            assert torch.equal(values[sl], alone[g].value(obs[sl]))
            start = policy_of(S.member_nets()[g])
            assert not torch.equal(start.act(obs[sl]), got[sl])       # the steps moved the weights
            start.close()
    finally:
        pset.close()
        for p in alone:
            p.close()

"""
rdv_lstm_ppo_set_loss_grad and ``LstmPolicySet.ppo_sequence_grads`` on the GPU (include/rdv.h, "Recurrent PPO minibatch gradients for
recurrent sets"; csrc/rdv_ppo_lstm.h, "the set form").  The specification is an equality: every output of member g — both flat
gradients, the eight scalars, log_prob, values — is, bit for bit, what rdv_lstm_ppo_loss_grad writes for a stand-alone ``LstmPolicy``
holding member g's weights, given the SAME full [T, N] buffer and ``envs = pieces[g]``.  So the comparison is ``torch.equal`` on the flat
buffers throughout.  The shapes are the smallest at which each mechanism can go wrong: a partial wave with a duplicate column, a lone
column beside a wider member (idle workgroups), 257 columns (two workgroups: the partial-sum order), every H, T = 1, a step where every
column is done, a long recurrence, absent members, the cap of 64 members.  One member is also held to the fp64 reference directly, under
the stand-alone call's rule and constants (tests/ppo_lstm_reference.py).
"""
import ctypes as C

import numpy as np
import pytest

import policy_lstm_reference as L
import policy_mlp_reference as M
import ppo_lstm_reference as Q
import ppo_lstm_set_helpers as S
from helpers import capture, gpu_batch
from policy_set_cases import short_episodes, stagger
from reinforcement_learning_rendezvous_amd import _native as N

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COEFS = dict(clip_range=Q.EPS, ent_coef=Q.ENT, vf_coef=Q.VF)

UNEVEN = (32, (64, 64), (64, 64), "tanh", "hot", (256, 256, 300), 5, "random")
UNEVEN_WIDTHS = (33, 1, 257)        # a partial wave with one duplicate; a lone column (idle workgroups beside the others); two workgroups


def make_set(case, backend="auto"):
    from reinforcement_learning_rendezvous_amd import LstmPolicySet
    return LstmPolicySet(S.make_members(case, DEV), list(case["sizes"]), backend=backend)


def flat_of(st, g=None):
    pick = (lambda t: t) if g is None else (lambda t: t[g])
    return torch.cat([pick(st["actor"]).reshape(-1), pick(st["critic"]).reshape(-1), pick(st["scalars"]).reshape(-1)]).clone()


def close_all(*things):
    for t in things:
        for p in (t if isinstance(t, (list, tuple)) else [t]):
            p.close()


def assert_members_equal_their_twins(case, lset, buf, pieces, res, **kw):
    """Every present member's five outputs against a stand-alone LstmPolicy of its weights on the same buffer and envs = pieces[g]."""
    dev = torch.device(DEV)
    twins = S.make_members(case, DEV)
    try:
        for g, piece in enumerate(pieces):
            if piece is None:
                assert res[g] is None
                continue
            want = twins[g].ppo_sequence_grad(buf, piece, **kw)
            torch.cuda.synchronize()
            assert torch.equal(flat_of(lset._ppo_seq[dev], g), flat_of(twins[g]._ppo_seq[dev])), f"member {g}: gradients or scalars"
            assert torch.equal(res[g]["log_prob"], want["log_prob"]) and torch.equal(res[g]["values"], want["values"]), f"member {g}"
            for k in ("loss", "approx_kl", "clip_fraction"):
                assert torch.equal(res[g][k], want[k])
            a, c = lset[g].lstm_actor.weight_hh_l0.grad, lset[g].lstm_critic.weight_ih_l0.grad
            assert a.data_ptr() == lset._ppo_seq[dev]["actor"][g].data_ptr() + 4 * 4 * case["H"] * 17      # .grad: views of the set's rows
            assert c.data_ptr() == lset._ppo_seq[dev]["critic"][g].data_ptr()
    finally:
        close_all(twins)


def run_case(args, widths, duplicate=None, **kw):
    case = S.make_set_case(*args)
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, widths, duplicate=duplicate, device=DEV)
    try:
        res = lset.ppo_sequence_grads(buf, pieces, **dict(COEFS, **kw))
        torch.cuda.synchronize()
        assert_members_equal_their_twins(case, lset, buf, pieces, res, **dict(COEFS, **kw))
    finally:
        close_all(lset.policies, lset)


@pytest.mark.parametrize("normalize", [True, False])
def test_uneven_members(normalize):
    run_case(UNEVEN, UNEVEN_WIDTHS, duplicate=0, normalize_advantage=normalize)


@pytest.mark.parametrize("H,pi,vf,act,cls", [(64, (32,), (32,), "relu", "hot"), (128, (64, 64), (32, 16), "tanh", "hot"),
                                             (256, (16, 16), (16, 16), "sigmoid", "default_init")])
def test_every_hidden_size(H, pi, vf, act, cls):
    run_case((H, pi, vf, act, cls, (256, 40), 3, "random"), (33, 1), normalize_advantage=False)


def test_one_step():
    run_case((32, (64, 64), (64, 64), "tanh", "default_init", (256, 300), 1, "random"), (256, 257), normalize_advantage=False)


def test_all_done():
    """A step where every column is done and a column (7 of the rollout: member 0's) done at every step."""
    case = S.make_set_case(32, (32, 16), (64,), "tanh", "hot", (256, 40), 4, "all_done")
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = [torch.tensor([7] + list(range(40, 72)), device=DEV), torch.arange(256, 289, device=DEV)]
    try:
        assert bool(buf["done"][1].all()) and bool(buf["done"][:, 7].all())
        res = lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, **COEFS)
        assert_members_equal_their_twins(case, lset, buf, pieces, res, normalize_advantage=False, **COEFS)
    finally:
        close_all(lset.policies, lset)


def test_long_memory():
    run_case((32, (64, 64), (32, 16), "tanh", "long_memory", (256, 40), 32, "sparse"), (33, 33), normalize_advantage=False)


def test_one_member_against_fp64():
    """Member 1 of the uneven case against Q.reference under the stand-alone rule err <= C max(e32, 2^-23), C = 32 / 128."""
    case = S.make_set_case(*UNEVEN)
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, UNEVEN_WIDTHS, duplicate=0, device=DEV)
    try:
        res = lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, **COEFS)
        torch.cuda.synchronize()
        st = lset._ppo_seq[torch.device(DEV)]
        actor, critic = case["nets"][1]
        got = Q.split_flat(st["actor"][1].cpu().numpy(), actor, True) + Q.split_flat(st["critic"][1].cpu().numpy(), critic, False)
        twin = dict(actor=actor, critic=critic)
        mb = S.member_minibatch(case, 1, pieces[1].cpu().numpy())
        ref64, ref32 = Q.reference(twin, "float64", mb=mb), Q.reference(twin, "float32", mb=mb)
        rows = Q.compare(Q.names(actor, critic), got, {k: float(res[1][k]) for k in Q.SCALARS}, ref64, ref32)
        for name, err, e32, C_ in rows:
            print(f"member 1 {name}: err {err:.3e} e32 {e32:.3e} ratio {err / max(e32, Q.FLOOR):.3f} (C {C_:g})")
        assert not Q.violations(rows), Q.violations(rows)
    finally:
        close_all(lset.policies, lset)


# ------------------------------------------------------------------------------------------------------------ the C call
class CCall:
    """rdv_lstm_ppo_set_loss_grad on buffers of its own: all five outputs filled with a sentinel in front of every call."""
    SENTINEL = 7.0

    def __init__(self, case, buf, P):
        from reinforcement_learning_rendezvous_amd.policy import ACTIVATIONS
        self.lib, self.case, self.buf, self.P = N.lib(), case, buf, P
        act = ACTIVATIONS[case["act"]][0]
        actor, critic = case["nets"][0]
        arch = lambda net: [int(w.shape[0]) for w in net["w"][:-1]]
        self.sa, self.sc = N.LstmSpec.make(case["H"], arch(actor), act), N.LstmSpec.make(case["H"], arch(critic), act)
        self.Ga, self.Gc = int(self.lib.rdv_lstm_ppo_grad_floats(C.byref(self.sa), 1)), int(self.lib.rdv_lstm_ppo_grad_floats(C.byref(self.sc), 0))
        self.ag, self.cg, self.sc8 = torch.zeros((P, self.Ga), device=DEV), torch.zeros((P, self.Gc), device=DEV), torch.zeros((P, 8), device=DEV)

    def need(self, counts):
        return int(self.lib.rdv_lstm_ppo_set_workspace_bytes(C.byref(self.sa), C.byref(self.sc), self.case["T"], len(counts), (C.c_int64 * len(counts))(*counts)))

    def __call__(self, actor, critic, envs, counts, short=0):
        p = lambda t: t.data_ptr()
        buf, T = self.buf, self.case["T"]
        total = int(sum(counts))
        self.lp, self.val = torch.empty(T * total, device=DEV), torch.empty(T * total, device=DEV)
        for t in (self.ag, self.cg, self.sc8, self.lp, self.val):
            t.fill_(self.SENTINEL)
        need = self.need(counts)
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rows = N.LstmPpoRows(p(buf["obs"]), p(buf["actions"]), p(buf["log_prob"]), p(buf["advantages"]), p(buf["returns"]), p(buf["done"]),
                             p(buf["lstm_state0"][0]), p(buf["lstm_state0"][1]), p(buf["lstm_critic_state0"][0]), p(buf["lstm_critic_state0"][1]),
                             p(envs), self.case["N"], T, total)
        out = N.LstmPpoSetOut(p(self.ag), p(self.cg), p(self.sc8), p(self.lp), p(self.val))
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        rc = self.lib.rdv_lstm_ppo_set_loss_grad(actor, critic, C.byref(rows), (C.c_int64 * len(counts))(*counts), Q.EPS, Q.ENT, Q.VF,
                                                 C.c_void_p(p(ws)), need - short, C.byref(out), stream)
        msg = self.lib.rdv_last_error().decode()
        torch.cuda.synchronize()
        return rc, msg

    def untouched(self):
        return all(bool((t == self.SENTINEL).all()) for t in (self.ag, self.cg, self.sc8, self.lp, self.val))

    def member(self, g, off, B):
        T = self.case["T"]
        return torch.cat([self.ag[g], self.cg[g], self.sc8[g], self.lp[T * off:T * (off + B)], self.val[T * off:T * (off + B)]]).clone()


def test_a_none_member_and_a_count_of_zero():
    case = S.make_set_case(*UNEVEN)
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, UNEVEN_WIDTHS, duplicate=0, device=DEV)
    try:
        st_of = lambda: lset._ppo_seq[torch.device(DEV)]
        full = lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, **COEFS)
        want = [flat_of(st_of(), g) for g in (0, 2)]
        # Python: member 1 sits the call out; its rows of the set's buffers keep a sentinel, the others' bits do not move
        for name in ("actor", "critic", "scalars"):
            st_of()[name][1].fill_(7.0)
        res = lset.ppo_sequence_grads(buf, [pieces[0], None, pieces[2]], normalize_advantage=False, **COEFS)
        torch.cuda.synchronize()
        assert res[1] is None and bool((flat_of(st_of(), 1) == 7.0).all())
        assert torch.equal(flat_of(st_of(), 0), want[0]) and torch.equal(flat_of(st_of(), 2), want[1])
        for g in (0, 2):
            assert torch.equal(res[g]["log_prob"], full[g]["log_prob"]) and torch.equal(res[g]["values"], full[g]["values"])
        # C: a count of 0 — nothing of the member is written, in any of the five outputs
        call = CCall(case, buf, 3)
        envs = torch.cat([pieces[0], pieces[2]])
        rc, msg = call(lset._handle("l", DEV), lset._handle("v", DEV), envs, [33, 0, 257])
        assert rc == 0, msg
        assert bool((torch.cat([call.ag[1], call.cg[1], call.sc8[1]]) == call.SENTINEL).all())
        assert torch.equal(call.member(0, 0, 33), torch.cat([want[0], full[0]["log_prob"].reshape(-1), full[0]["values"].reshape(-1)]))
        assert torch.equal(call.member(2, 33, 257), torch.cat([want[1], full[2]["log_prob"].reshape(-1), full[2]["values"].reshape(-1)]))
    finally:
        close_all(lset.policies, lset)


def test_a_plain_handle_pair_is_a_set_of_one():
    case = S.make_set_case(32, (64, 64), (64, 64), "tanh", "hot", (300,), 3, "random")
    pol, buf = S.make_members(case, DEV)[0], S.make_buf(case, DEV)
    envs = S.pieces_of(case, (257,), device=DEV)[0]
    try:
        want = pol.ppo_sequence_grad(buf, envs, normalize_advantage=False, **COEFS)
        torch.cuda.synchronize()
        call = CCall(case, buf, 1)
        rc, msg = call(pol._handle("l", DEV), pol._handle("v", DEV), envs, [257])
        assert rc == 0, msg
        assert torch.equal(call.member(0, 0, 257), torch.cat([flat_of(pol._ppo_seq[torch.device(DEV)]), want["log_prob"].reshape(-1), want["values"].reshape(-1)]))
    finally:
        pol.close()


def test_the_cap_of_64_members():
    sizes = (256,) * 63 + (1,)
    case = S.make_set_case(32, (16,), (16,), "tanh", "hot", sizes, 2, "random")
    assert case["N"] == 63 * 256 + 1
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, (1,) * 64, device=DEV)
    dev = torch.device(DEV)
    big = None
    try:
        res = lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, **COEFS)
        torch.cuda.synchronize()
        got = [flat_of(lset._ppo_seq[dev], g) for g in range(64)]
        lp = [res[g]["log_prob"].clone() for g in range(64)]
        for g in range(64):                                   # the member modules serve as their own stand-alone twins here
            want = lset[g].ppo_sequence_grad(buf, pieces[g], normalize_advantage=False, **COEFS)
            assert torch.equal(got[g], flat_of(lset[g]._ppo_seq[dev])) and torch.equal(lp[g], want["log_prob"]), f"member {g}"
        # 65 members: refused, nothing enqueued
        from reinforcement_learning_rendezvous_amd import LstmPolicy, LstmPolicySet
        extra = LstmPolicy(L.weights_dict(*case["nets"][0]), activation_fn=case["act"], n_rows=1).to(DEV)
        big = LstmPolicySet(list(lset.policies) + [extra], [256] * 64 + [1])
        call = CCall(case, buf, 64)
        rc, msg = call(big._handle("l", DEV), big._handle("v", DEV), torch.cat(pieces), [1] * 64)
        assert rc == -1 and "65 members" in msg and "at most 64" in msg and call.untouched(), msg
    finally:
        close_all(lset.policies, lset)
        if big is not None:
            close_all(big, extra)


def test_refusals_at_the_handle_stage():
    from reinforcement_learning_rendezvous_amd import LstmPolicy, LstmPolicySet, MlpPolicy, PolicySet
    case = S.make_set_case(32, (32,), (16,), "tanh", "hot", (256, 256, 40), 3, "random")
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, (2, 2, 2), device=DEV)
    envs, counts = torch.cat(pieces), [2, 2, 2]
    two = LstmPolicySet(list(lset.policies[:2]), [256, 40])
    other_h = [LstmPolicy(L.weights_dict(L.hot(64, (32,), "tanh", seed=g), L.critic_of(L.hot(64, (16,), "tanh", seed=9 + g))), activation_fn="tanh", n_rows=1).to(DEV)
               for g in range(3)]
    other = LstmPolicySet(other_h, [256, 256, 40])
    nets = [M.dense([32], "tanh", seed=5 + g) for g in range(3)]
    mlps = [MlpPolicy(M.weights_dict(n, M.critic_of(M.dense([16], "tanh", seed=20 + g))), activation_fn="tanh").to(DEV) for g, n in enumerate(nets)]
    mset = PolicySet(mlps, [256, 256, 40])
    try:
        call = CCall(case, buf, 3)
        a, v = lset._handle("l", DEV), lset._handle("v", DEV)
        rc, msg = call(a, v, envs, counts)
        assert rc == 0 and not call.untouched(), msg
        for args, word in (((v, a), "swapped"), ((mset._hip_handle(DEV), v), "not a recurrent"), ((a, two._handle("v", DEV)), "3 members, critic_set has 2"),
                           ((a, other._handle("v", DEV)), "hidden_size")):
            rc, msg = call(*args, envs, counts)
            assert rc == -1 and word in msg and call.untouched(), (word, msg)
        rc, msg = call(a, v, envs, counts, short=16)
        assert rc == -1 and "workspace_bytes" in msg and call.untouched(), msg
        rc, msg = call(None, v, envs, [6])
        assert rc == -5 and call.untouched()
    finally:
        close_all(lset.policies, lset, two, other_h, other, mlps, mset)


# ------------------------------------------------------------------------------------------------------------ determinism, stream order
def test_two_calls_agree_and_a_replayed_graph_equals_eager():
    case = S.make_set_case(*UNEVEN)
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, UNEVEN_WIDTHS, duplicate=0, device=DEV)
    dev = torch.device(DEV)
    try:
        call = lambda: lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, check=False, **COEFS)   # (the check reads the pieces on the host)
        first = call(); a = flat_of(lset._ppo_seq[dev])
        second = call(); b = flat_of(lset._ppo_seq[dev])
        assert torch.equal(a, b)
        assert all(torch.equal(first[g][k], second[g][k]) for g in range(3) for k in ("log_prob", "values"))
        kept = {}
        graph = capture(lambda: kept.update(res=call()))
        st = lset._ppo_seq[dev]
        for _ in range(2):
            st["actor"].fill_(float("nan")); st["critic"].fill_(float("nan"))
            for g in range(3):
                kept["res"][g]["values"].fill_(float("nan")); kept["res"][g]["log_prob"].fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(flat_of(st)[:-3 * 8], a[:-3 * 8])
            assert all(torch.equal(kept["res"][g][k], first[g][k]) for g in range(3) for k in ("log_prob", "values"))
    finally:
        close_all(lset.policies, lset)


def test_state_and_flags_are_untouched_and_a_members_new_weights_are_differentiated():
    case = S.make_set_case(*UNEVEN)
    lset, buf = make_set(case), S.make_buf(case, DEV)
    pieces = S.pieces_of(case, UNEVEN_WIDTHS, duplicate=0, device=DEV)
    dev, n, H = torch.device(DEV), case["N"], case["H"]
    fresh = None
    try:
        lset.state = (torch.full((n, H), 0.25, device=DEV), torch.full((n, H), -0.5, device=DEV))
        lset.critic_state = (torch.full((n, H), -0.125, device=DEV), torch.full((n, H), 0.75, device=DEV))
        flags = (torch.arange(n, device=DEV) % 3 == 0).to(torch.uint8)
        lset._set_pending("l", flags, DEV); lset._set_pending("v", flags, DEV)
        snapshot = lambda: [t.clone() for t in (*lset.state, *lset.critic_state, *lset.state_at_start("l", DEV), *lset.state_at_start("v", DEV))]
        before = snapshot()
        call = lambda: lset.ppo_sequence_grads(buf, pieces, normalize_advantage=False, **COEFS)
        call()
        old = [flat_of(lset._ppo_seq[dev], g) for g in range(3)]
        assert all(torch.equal(x, y) for x, y in zip(before, snapshot()))
        # behind rdv_lstm_set_member_weights for member 1 on the same stream: its new block is differentiated, members 0 and 2 keep their bits
        actor, critic = case["nets"][1]
        w = L.weights_dict(actor, critic)
        w = {k: (np.asarray(v) * np.float32(0.5) if k.endswith("weight_hh_l0") or k.startswith("action_net") else v) for k, v in w.items()}
        from reinforcement_learning_rendezvous_amd import LstmPolicy
        fresh = LstmPolicy(w, activation_fn=case["act"], n_rows=1).to(DEV)
        lset.update_weights(member=1, weights=w)
        call()
        fresh.ppo_sequence_grad(buf, pieces[1], normalize_advantage=False, **COEFS)
        torch.cuda.synchronize()
        new = [flat_of(lset._ppo_seq[dev], g) for g in range(3)]
        assert torch.equal(new[0], old[0]) and torch.equal(new[2], old[2])
        assert torch.equal(new[1], flat_of(fresh._ppo_seq[dev])) and not torch.equal(new[1], old[1])
    finally:
        close_all(lset.policies, lset)
        if fresh is not None:
            fresh.close()


# ------------------------------------------------------------------------------------------------------------ the learner loop
def test_two_update_steps_end_to_end_beside_stand_alone_twins():
    """collect(set) -> ppo_sequence_grads -> per member clip_grad_norm_ + torch.optim.Adam -> update_weights(member=g), twice; beside it
    stand-alone twins that take ppo_sequence_grad on the set's buffers with the same optimiser: gradients and parameters bit for bit."""
    from reinforcement_learning_rendezvous_amd import LstmPolicy, LstmPolicySet, ppo
    sizes, T, H = [256, 64], 8, 32
    nets = []
    for g in range(2):
        a = L.hot(H, (64, 64), "tanh", seed=3 + g)
        a["log_std"] = np.full(6, -0.7, np.float32)
        nets.append((a, L.critic_of(L.hot(H, (64, 64), "tanh", seed=52 + g))))
    make = lambda g, m: LstmPolicy(L.weights_dict(*nets[g]), activation_fn="tanh", n_rows=m).to(DEV)
    members, twins = [make(g, m) for g, m in enumerate(sizes)], [make(g, 1) for g in range(2)]
    lset = LstmPolicySet(members, sizes, seed=5)
    env = gpu_batch(sum(sizes), params=short_episodes(), seed=13)
    try:
        env.reset()
        stagger(env)
        params = lambda p: [t for group in ppo._sequence_params(p) for t in group]
        opts = []
        for p in members + twins:
            for t in params(p):
                t.requires_grad_(True)
            opts.append(torch.optim.Adam(params(p), lr=1e-3))
        gen = torch.Generator(device=DEV).manual_seed(1)
        for step in range(2):
            buf = env.collect(lset, T, gamma=0.97, gae_lambda=0.92)
            pieces = ppo.ppo_sequence_set_minibatches(lset, 33, gen)[0]
            res = lset.ppo_sequence_grads(buf, pieces, clip_range=0.2, ent_coef=Q.ENT, vf_coef=Q.VF)
            for g in range(2):
                want = twins[g].ppo_sequence_grad(buf, pieces[g], clip_range=0.2, ent_coef=Q.ENT, vf_coef=Q.VF)
                for a, b in zip(params(members[g]), params(twins[g])):
                    assert torch.equal(a.grad, b.grad), f"step {step} member {g}: gradients"
                assert torch.equal(res[g]["values"], want["values"]) and torch.equal(res[g]["loss"], want["loss"])
                for p, opt in ((members[g], opts[g]), (twins[g], opts[2 + g])):
                    torch.nn.utils.clip_grad_norm_(params(p), 0.5)
                    opt.step()
                lset.update_weights(member=g)
                twins[g].update_weights()
                for a, b in zip(params(members[g]), params(twins[g])):
                    assert torch.equal(a, b), f"step {step} member {g}: parameters"
        assert bool(buf["done"].any()) and bool(buf["lstm_state0"][0].any())
    finally:
        close_all(members, twins, lset)
        env.close()

"""
GPU: rdv_ppo_mlp_set_adam_step (include/rdv.h, "Gradient clip, Adam and weight repack for policy sets of every MLP architecture";
csrc/rdv_ppo_adam.h) and PolicySet.adam_step of sets of other architectures than the shipped one.

The rules are those of tests/test_gpu_ppo_adam.py, with its references (tests/ppo_adam_reference.py) as they are: ``coef`` within 1 ulp
of ``coef32`` and ``clip_coef`` exactly 1 where PyTorch's is; parameters and both moments bit for bit ``step32`` given the stored
``coef``; parameters against ``step64`` within ``bound``, which is counted per entry and so carries over to any length; the repacked
blocks against stand-alone rdv_policy_create_mlp / rdv_critic_create_mlp handles made from the stepped parameters, byte for byte but for
the six exp(log_std) floats (within 1 ulp).  Sets, members and rows: tests/ppo_mlp_set_helpers.py.  The sets are driven through
``PolicySet.ppo_grads`` / ``adam_step`` (one library call each); where a test needs gradients of its own it writes them into the
gradient buffers the set owns, which is what the call reads.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_reference as M
import ppo_adam_reference as A
import ppo_mlp_set_helpers as H
import ppo_reference as P
import test_ppo_set_grad as S
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd import ppo
from reinforcement_learning_rendezvous_amd.policy import MlpPolicy, PolicySet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = torch.device(DEV)
ENT, VF = 0.01, 0.5
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
GRAD_CASES = A.GRAD_CASES
NAMES = ("actor_param", "critic_param", "actor_m", "actor_v", "critic_m", "critic_v")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_bytes(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


def columns(pair):
    return {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in H.columns(pair).items()}


gradients = A.gradients


def ready(pset, cols, counts=(64, 40, 64)):
    """One ppo_grads so that the set owns its gradient buffers on the device, then its optimiser state -> (gradient state, Adam state)"""
    idx = [H.member_indices(g, n).to(DEV) if n else None for g, n in enumerate(counts)]
    pset.ppo_grads(H.make_buf(cols), idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
    assert ppo.hip_set_route(pset) == "mlp" and ppo._adam_device(pset) == D
    return pset._ppo[D], ppo._adam_state(pset, D)


def snapshot(pset, ad):
    out = {k: ad[k].cpu().numpy().copy() for k in NAMES + ("step", "coef")}
    out["blocks"] = [blocks(pset, g) for g in range(len(pset))]
    return out


def blocks(pset, g):
    """[actor block, critic block] of member g of the set's handles"""
    return [A.read_block(h, g) for h in (pset._hip_handle(DEV), pset._critic_handle(DEV))]


def blocks_equal(got, want, actor):
    """ppo_adam_reference.blocks_equal's rule for a block of pack_mlp_weights"""
    return A.blocks_equal(got, want, actor, A.MLP_STD)


def fresh(member):
    """A freshly packed stand-alone policy of the member's state_dict(): rdv_policy_create_mlp / rdv_critic_create_mlp on its weights"""
    sd = {k: v.detach().cpu().numpy().copy() for k, v in member.state_dict().items()}
    layers = lambda prefix, n: ([sd[f"{prefix}{i + 1}.weight"] for i in range(n)], [sd[f"{prefix}{i + 1}.bias"] for i in range(n)])
    actor = M.make_net(*layers("l", len(member.pi_arch) + 1), member.activation, sd["log_std"])
    critic = M.make_net(*layers("v", len(member.vf_arch) + 1), member.activation)
    return H.policy_of((actor, critic)).to(DEV)


def assert_blocks_are_the_host_packers(pset, members):
    for g in members:
        alone = fresh(pset[g])
        try:
            for got, want, actor in zip(blocks(pset, g), blocks(alone, 0), (True, False)):
                assert blocks_equal(got, want, actor) is None, (g, actor, blocks_equal(got, want, actor))
        finally:
            alone.close()


@pytest.mark.parametrize("key", ["a", "b", "d"])
def test_consecutive_steps_hold_the_restatement_bit_for_bit_and_the_float64_bound(key):
    """P = 3, member 1 inactive; one gradient case per step (zero first: with zero moments nothing moves), so members step from non-zero
    moments too."""
    pair = H.PAIRS[key]
    pset = H.make_set(pair).to(DEV)
    try:
        st, ad = ready(pset, columns(pair))
        ga_n, gc_n = int(st["actor"].shape[1]), int(st["critic"].shape[1])
        nets = H.member_nets(pair)
        for g in range(3):
            assert np.array_equal(ad["actor_param"][g].cpu().numpy(), H.flat(nets[g][0])) and np.array_equal(ad["critic_param"][g].cpu().numpy(), H.flat(nets[g][1]))
        p64 = {g: [ad["actor_param"][g].cpu().numpy().astype(np.float64), ad["critic_param"][g].cpu().numpy().astype(np.float64)] for g in (0, 2)}
        m64 = {g: [np.zeros(ga_n), np.zeros(gc_n)] for g in (0, 2)}
        v64 = {g: [np.zeros(ga_n), np.zeros(gc_n)] for g in (0, 2)}
        tol = {g: [np.zeros(ga_n), np.zeros(gc_n)] for g in (0, 2)}
        dmax = {g: [np.zeros(ga_n), np.zeros(gc_n)] for g in (0, 2)}
        for k, (name, scale, max_norm) in enumerate(GRAD_CASES):
            grads = [gradients(10 * k + g, scale, ga_n, gc_n) for g in range(3)]
            st["actor"].copy_(torch.from_numpy(np.stack([g[0] for g in grads])))
            st["critic"].copy_(torch.from_numpy(np.stack([g[1] for g in grads])))
            before = snapshot(pset, ad)
            res = pset.adam_step([{}, None, {}], lr=LR, betas=(B1, B2), eps=EPS, max_grad_norm=max_norm)
            torch.cuda.synchronize()
            after = snapshot(pset, ad)
            for n in NAMES + ("step", "coef"):                       # the inactive member: byte-identical rows and blocks
                assert same_bytes(before[n][1], after[n][1]), (name, n)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before["blocks"][1], after["blocks"][1]))
            for g in (0, 2):
                coef = after["coef"][g]
                want = A.coef64(grads[g][0], grads[g][1], k, LR, B1, B2, max_norm)
                assert all(A.within_ulps(coef[i], want[i]) for i in range(4)), (name, g, coef, want)
                assert np.array_equal(coef[4:], np.zeros(4, np.float32)) and after["step"][g] == k + 1
                assert float(res["total_norm"][g]) == coef[0] and float(res["skipped"][g]) == 0.0
                if name in ("zero", "unclipped", "no_clipping"):
                    assert coef[1] == 1.0, (name, coef)              # PyTorch's clamp: exactly 1
                else:
                    assert coef[1] < 1.0
                for kind, gi in (("actor", 0), ("critic", 1)):
                    p, m, v = A.step32(before[kind + "_param"][g], before[kind + "_m"][g], before[kind + "_v"][g], grads[g][gi], coef, B1, B2, EPS)
                    for n, w in ((kind + "_param", p), (kind + "_m", m), (kind + "_v", v)):
                        assert np.array_equal(after[n][g].view(np.uint32), w.view(np.uint32)), (name, g, n)
                moved = not np.array_equal(before["actor_param"][g], after["actor_param"][g])
                assert moved == (name != "zero"), (name, g)
                pa, pc, ma, mc, va, vc, d = A.step64(p64[g][0], p64[g][1], m64[g][0], m64[g][1], v64[g][0], v64[g][1], grads[g][0], grads[g][1],
                                                     k, LR, B1, B2, EPS, max_norm)
                p64[g], m64[g], v64[g] = [pa, pc], [ma, mc], [va, vc]
                for i, n in enumerate(("actor_param", "critic_param")):
                    dmax[g][i] = np.maximum(dmax[g][i], d[i])
                    tol[g][i] = tol[g][i] + A.bound(p64[g][i], dmax[g][i])
                    err = np.abs(after[n][g].astype(np.float64) - p64[g][i])
                    assert (err <= tol[g][i]).all(), (name, g, n, float((err / np.maximum(tol[g][i], 1e-300)).max()))
            assert_blocks_are_the_host_packers(pset, (0, 2))
    finally:
        pset.close()


def corner(nets, which, layer):
    """ppo_adam_reference.corner_nets' four corners applied to layer ``layer`` of both nets (0-based; the last: the head)"""
    f32 = np.float32
    out = []
    for net in nets:
        net = dict(net, w=[x.copy() for x in net["w"]], b=[x.copy() for x in net["b"]])
        w = net["w"]
        if which == "cross":
            w[layer][0, 1] = f32(32.0 - 1e-4)
        elif which == "big":
            w[0][5, 2], w[layer][0, 3] = f32(40.0), f32(-3000.0)
        elif which == "tiny":
            w[layer] = (w[layer] * f32(2.0 ** -19)).astype(np.float32)
        elif which == "zero":
            w[layer] = np.zeros_like(w[layer]); net["b"][layer] = np.zeros_like(net["b"][layer])
            w[0][0, 0] = f32(-0.0)
        out.append(net)
    return tuple(out)


CORNER_CASES = [(((32, 32), (32, 32), "relu"), 1), (((32, 32), (32, 32), "relu"), 2), (((16, 64), (16, 64), "tanh"), 1), (((16, 64), (16, 64), "tanh"), 2)]


@pytest.mark.parametrize("pair,layer", CORNER_CASES, ids=["a-hidden", "a-head", "16x64-hidden", "16x64-head"])
def test_repacked_blocks_are_the_host_packers_at_its_corners(pair, layer):
    """Members 0..3 carry the corners "cross", "big", "tiny", "zero" in one layer; after a step the blocks equal stand-alone handles of
    the stepped parameters, and deterministic actions, values and the gradients on the repacked set equal those handles'."""
    nets = [corner(n, which, layer) for n, which in zip(H.member_nets(pair, 4), A.CORNERS)]
    sizes = [256, 256, 256, 432]
    starts = [0, 256, 512, 768]
    pset = PolicySet([H.policy_of(n) for n in nets], sizes).to(DEV)
    cols = columns(pair)
    buf = H.make_buf(cols)
    idx = [torch.from_numpy(starts[g] + np.random.default_rng([3, g]).permutation(sizes[g])[:100].astype(np.int64)).to(DEV) for g in range(4)]
    try:
        stepped = pset.ppo_grads(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
        st, ad = pset._ppo[D], ppo._adam_state(pset, D)
        ga_n, gc_n = int(st["actor"].shape[1]), int(st["critic"].shape[1])
        grads = [gradients(70 + g, 3.0, ga_n, gc_n) for g in range(4)]   # every entry moves by about lr
        st["actor"].copy_(torch.from_numpy(np.stack([g[0] for g in grads])))
        st["critic"].copy_(torch.from_numpy(np.stack([g[1] for g in grads])))
        before = ad["actor_param"].clone()
        pset.adam_step(stepped, lr=LR, eps=EPS, max_grad_norm=0.5)
        torch.cuda.synchronize()
        assert not bits_equal(before, ad["actor_param"])
        assert_blocks_are_the_host_packers(pset, range(4))
        obs = cols["obs"]
        got, values = pset.act(obs), pset.value(obs)
        out = pset.ppo_grads(buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
        for g, sl in enumerate(pset.group_slices):
            alone = fresh(pset[g])
            try:
                assert torch.equal(got[sl], alone.act(obs[sl])) and torch.equal(values[sl], alone.value(obs[sl])), g
                s = alone.ppo_grad(buf, idx[g], clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
                for (name, x), y in zip(pset[g].named_parameters(), alone.parameters()):
                    assert bits_equal(x.grad, y.grad), (g, name)
                assert all(bits_equal(out[g][k], s[k]) for k in s)
            finally:
                alone.close()
    finally:
        pset.close()


def test_members_with_a_nan_or_an_infinite_gradient_are_skipped_whole_and_flagged():
    pair = H.PAIRS["a"]
    pset = H.make_set(pair).to(DEV)
    try:
        st, ad = ready(pset, columns(pair))
        pset.adam_step(None, lr=LR, eps=EPS, max_grad_norm=0.5)        # moments and steps are not zero when the bad gradients arrive
        st["actor"][0, 17] = float("nan")
        st["critic"][2, 5] = float("-inf")
        before = snapshot(pset, ad)
        res = pset.adam_step(None, lr=LR, eps=EPS, max_grad_norm=0.5)
        torch.cuda.synchronize()
        after = snapshot(pset, ad)
        for g in (0, 2):
            for n in NAMES + ("step",):
                assert same_bytes(before[n][g], after[n][g]), (g, n)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before["blocks"][g], after["blocks"][g]))
            assert after["coef"][g][4] == 1.0 and float(res["skipped"][g]) == 1.0 and not np.isfinite(after["coef"][g][0])
        assert after["step"][1] == 2 and after["coef"][1][4] == 0.0 and not np.array_equal(before["actor_param"][1], after["actor_param"][1])
        assert_blocks_are_the_host_packers(pset, (1,))
    finally:
        pset.close()


def test_an_act_queued_before_the_step_reads_the_old_block_and_one_after_the_new():
    pair = H.PAIRS["a"]
    pset = H.make_set(pair).to(DEV)
    cols = columns(pair)
    try:
        ready(pset, cols)
        obs = cols["obs"]
        old = [fresh(m) for m in pset]
        a0 = pset.act(obs)
        pset.adam_step(None, lr=1e-2, eps=EPS, max_grad_norm=0.5)
        a1 = pset.act(obs)
        torch.cuda.synchronize()
        for g, sl in enumerate(pset.group_slices):
            new = fresh(pset[g])
            assert torch.equal(a0[sl], old[g].act(obs[sl])) and torch.equal(a1[sl], new.act(obs[sl])) and not torch.equal(a0[sl], a1[sl]), g
            new.close(); old[g].close()
    finally:
        pset.close()


def c_pair(pset, st, ad, counts, lr=LR, max_norm=0.5):
    """The two library calls on the set's own buffers (the indices and the workspace of its last ppo_grads), as one function that enqueues
    on the current stream"""
    lib = N.lib()
    cnt = (C.c_int64 * len(counts))(*counts)
    buf = pset._test_buf
    rows = N.PpoRows(buf["obs"].data_ptr(), buf["actions"].data_ptr(), buf["log_prob"].data_ptr(), buf["advantages"].data_ptr(), buf["returns"].data_ptr(),
                     st["idx"].data_ptr(), P.ROWS)
    out = N.PpoSetOut(st["actor"].data_ptr(), st["critic"].data_ptr(), st["scalars"].data_ptr(), None, None)
    a, c = pset._hip_handle(DEV), pset._critic_handle(DEV)
    mask = C.c_uint64((1 << len(counts)) - 1)

    def run():
        s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        N.check(lib.rdv_ppo_mlp_set_loss_grad(a, c, C.byref(rows), cnt, P.EPS, ENT, VF, C.c_void_p(st["workspace"].data_ptr()), st["workspace"].numel(), C.byref(out), s))
        N.check(lib.rdv_ppo_mlp_set_adam_step(a, c, C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()), C.c_void_p(st["critic"].data_ptr()), mask, lr, B1, B2, EPS,
                                              max_norm, s))
    run.keep = (cnt, rows, out)
    return run


def test_three_replays_of_a_captured_grads_plus_step_pair_equal_three_eager_iterations():
    pair, counts = H.PAIRS["b"], (127, 257, 128)
    cols = columns(pair)
    sets = [H.make_set(pair).to(DEV) for _ in range(2)]
    try:
        runs = []
        for pset in sets:
            pset._test_buf = H.make_buf(cols)
            idx = [H.member_indices(g, n).to(DEV) for g, n in enumerate(counts)]
            pset.ppo_grads(pset._test_buf, idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF, normalize_advantage=False)
            runs.append(c_pair(pset, pset._ppo[D], ppo._adam_state(pset, D), counts))
        for _ in range(3):
            runs[0]()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                runs[1]()
            for _ in range(3):
                g.replay()
            stream.synchronize()
        torch.cuda.synchronize()
        x, y = (snapshot(s, ppo._adam_state(s, D)) for s in sets)
        for n in NAMES + ("step", "coef"):
            assert same_bytes(x[n], y[n]), n
        assert list(x["step"]) == [3, 3, 3]
        for bx, by in zip(x["blocks"], y["blocks"]):
            assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(bx, by))
        assert bits_equal(sets[0]._ppo[D]["actor"], sets[1]._ppo[D]["actor"])
    finally:
        for s in sets:
            s.close()


def test_default_spec_sets_get_the_bits_of_the_shipped_call_and_refusals_enqueue_nothing():
    cols = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in S.set_columns().items()}
    sets = [S.make_set().to(DEV) for _ in range(2)]
    general = H.make_set(H.PAIRS["a"]).to(DEV)
    two = PolicySet([H.policy_of(n) for n in H.member_nets(H.PAIRS["a"], 2)], [256, 944]).to(DEV)
    try:
        lib = N.lib()
        ads = []
        for pset in sets:
            idx = [S.member_indices(g, 64).to(DEV) for g in range(3)]
            pset.ppo_grads(H.make_buf(cols), idx, clip_range=P.EPS, ent_coef=ENT, vf_coef=VF)
            ads.append(ppo._adam_state(pset, D))
        for pset, ad, fn in zip(sets, ads, ("rdv_ppo_mlp_set_adam_step", "rdv_ppo_set_adam_step")):
            st = pset._ppo[D]
            N.check(getattr(lib, fn)(pset._hip_handle(DEV), pset._critic_handle(DEV), C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()),
                                     C.c_void_p(st["critic"].data_ptr()), C.c_uint64(5), LR, B1, B2, EPS, 0.5, None))
        torch.cuda.synchronize()
        x, y = (snapshot(s, a) for s, a in zip(sets, ads))
        for n in NAMES + ("step", "coef"):
            assert same_bytes(x[n], y[n]), n
        assert list(x["step"]) == [1, 0, 1]
        # handle-level refusals of the general call: nothing is enqueued, the state stays
        st, ad = ready(general, columns(H.PAIRS["a"]))
        before = snapshot(general, ad)
        a, c = general._hip_handle(DEV), general._critic_handle(DEV)
        for handles, words in (((sets[0]._hip_handle(DEV), c), ("actor_set has the default spec", "mixed pair")),
                               ((a, sets[0]._critic_handle(DEV)), ("critic_set has the default spec", "mixed pair")),
                               ((c, a), ("swapped",)),
                               ((a, two._critic_handle(DEV)), ("actor_set has 3 members", "critic_set has 2"))):
            rc = lib.rdv_ppo_mlp_set_adam_step(handles[0], handles[1], C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()), C.c_void_p(st["critic"].data_ptr()),
                                               C.c_uint64(7), LR, B1, B2, EPS, 0.5, None)
            msg = lib.rdv_last_error().decode()
            assert rc == -1 and all(w in msg for w in words) and "rdv_ppo_mlp_set_adam_step" in msg, (words, rc, msg)
        torch.cuda.synchronize()
        after = snapshot(general, ad)
        for n in NAMES + ("step", "coef"):
            assert same_bytes(before[n], after[n]), n
    finally:
        for s in sets + [general, two]:
            s.close()


def test_three_update_steps_end_to_end_without_update_weights():
    """collect -> ppo_grads -> adam_step on a [32, 32] ReLU set of three members of 256 envs, T = 4, three minibatch steps, no
    update_weights(): each member's parameters stay within the counted bound of a float64 learner (PyTorch's clip_grad_norm_ and Adam
    on float64 copies, fed the same gradients), and after each step the set's deterministic actions are those of a freshly packed
    MlpPolicy of the member's state_dict().  On the parent the forward blocks stay stale without update_weights(), and the last
    assertion fails."""
    from helpers import gpu_batch
    from reinforcement_learning_rendezvous_amd import ppo_set_minibatches
    pair = H.PAIRS["a"]
    pset = PolicySet([H.policy_of(n) for n in H.member_nets(pair)], [256, 256, 256])
    env = gpu_batch(768, seed=11)
    try:
        env.reset()
        buf = env.collect(pset, 4, gamma=0.99, gae_lambda=0.95)
        obs = buf["obs"][0]
        assert ppo.hip_set_route(pset) == "mlp"
        twins = [[torch.nn.Parameter(p.detach().to("cpu", torch.float64).clone()) for p in m.parameters()] for m in pset]
        opts = [torch.optim.Adam(t, lr=LR, eps=EPS) for t in twins]
        tol = [[np.zeros(tuple(p.shape)) for p in t] for t in twins]
        dmax = [[np.zeros(tuple(p.shape)) for p in t] for t in twins]
        start = pset.act(obs).clone()
        steps = ppo_set_minibatches(pset, 4, 400, torch.Generator(device=DEV).manual_seed(3))
        assert len(steps) == 3
        for k, pieces in enumerate(steps):
            stepped = pset.ppo_grads(buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
            grads = [[p.grad.detach().to("cpu", torch.float64).clone() for p in m.parameters()] for m in pset]
            out = pset.adam_step(stepped, lr=LR, eps=EPS, max_grad_norm=0.5)
            assert not bool(out["skipped"].any()) and bool((out["total_norm"] > 0).all())
            for g in range(3):
                m_before = [opts[g].state[p]["exp_avg"].numpy().copy() if p in opts[g].state else np.zeros(tuple(p.shape)) for p in twins[g]]
                for p, gr in zip(twins[g], grads[g]):
                    p.grad = gr.clone()
                torch.nn.utils.clip_grad_norm_(twins[g], 0.5)
                gp = [p.grad.numpy().copy() for p in twins[g]]
                opts[g].step()
                step_size, bc2 = LR / (1.0 - B1 ** (k + 1)), 1.0 - B2 ** (k + 1)
                for i, (p, q) in enumerate(zip(twins[g], pset[g].parameters())):
                    state = opts[g].state[p]
                    den = np.sqrt(state["exp_avg_sq"].numpy()) / np.sqrt(bc2) + EPS
                    d = step_size * (np.abs(state["exp_avg"].numpy()) + (1.0 - B1) * (np.abs(gp[i]) + np.abs(m_before[i]))) / den   # step64's scale
                    dmax[g][i] = np.maximum(dmax[g][i], d)
                    tol[g][i] = tol[g][i] + A.bound(p.detach().numpy(), dmax[g][i])
                    err = np.abs(q.detach().cpu().numpy().astype(np.float64) - p.detach().numpy())
                    assert (err <= tol[g][i]).all(), (k, g, i, float((err / tol[g][i]).max()))
            got = pset.act(obs)
            for g, sl in enumerate(pset.group_slices):
                alone = fresh(pset[g])
                assert torch.equal(got[sl], alone.act(obs[sl])), (k, g)
                alone.close()
        assert pset._adam[D]["step"].tolist() == [3, 3, 3] and not torch.equal(start, pset.act(obs))
    finally:
        pset.close(); env.close()

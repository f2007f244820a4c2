"""
CPU tests of the recurrent set's PPO minibatch gradients (include/rdv.h, "Recurrent PPO minibatch gradients for recurrent sets"): the
workspace sum rule of rdv_lstm_ppo_set_workspace_bytes, the host-only refusals of rdv_lstm_ppo_set_loss_grad in their stated order,
``ppo_sequence_set_minibatches``, and ``LstmPolicySet.ppo_sequence_grads``' PyTorch fallback, which equals the members' own
``ppo_sequence_grad(backend="torch")`` by equality.  No GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_lstm_reference as Q
import ppo_lstm_set_helpers as S
import reinforcement_learning_rendezvous_amd as pkg
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd import ppo
from reinforcement_learning_rendezvous_amd.policy import ACTIVATIONS
from reinforcement_learning_rendezvous_amd.policy_lstm import LstmPolicySet

COEFS = dict(clip_range=Q.EPS, ent_coef=Q.ENT, vf_coef=Q.VF)


def spec(H, arch, act="tanh"):
    return N.LstmSpec.make(H, arch, ACTIVATIONS[act][0])


def counts_of(values):
    return (C.c_int64 * len(values))(*values)


# ------------------------------------------------------------------------------------------------------------ the C ABI, host only
def test_workspace_bytes_is_the_sum_of_the_members():
    lib = N.lib()
    a, c = spec(64, [64, 64]), spec(64, [32])
    one = lambda T, B: int(lib.rdv_lstm_ppo_workspace_bytes(C.byref(a), C.byref(c), T, B))
    many = lambda T, counts: int(lib.rdv_lstm_ppo_set_workspace_bytes(C.byref(a), C.byref(c), T, len(counts), counts_of(counts)))
    for T in (1, 5, 128):
        for counts in ([1], [33, 1, 257], [0, 33, 0, 1], [256, 0, 0], [0, 0, 7], [5000, 31, 32, 0, 255]):
            want = sum(one(T, B) for B in counts if B > 0)
            assert many(T, counts) == want and want % 16 == 0, (T, counts)
    # -1: a bad pair of specs, n_steps <= 0, n_members outside 1..64, null counts, a negative count, no positive count
    assert int(lib.rdv_lstm_ppo_set_workspace_bytes(C.byref(a), C.byref(spec(32, [32])), 4, 1, counts_of([4]))) == -1
    assert int(lib.rdv_lstm_ppo_set_workspace_bytes(None, C.byref(c), 4, 1, counts_of([4]))) == -1
    assert many(0, [4]) == -1 and many(-2, [4]) == -1
    assert int(lib.rdv_lstm_ppo_set_workspace_bytes(C.byref(a), C.byref(c), 4, 0, counts_of([4]))) == -1
    assert many(4, [1] * 65) == -1 and many(4, [1] * 64) == 64 * one(4, 1)
    assert int(lib.rdv_lstm_ppo_set_workspace_bytes(C.byref(a), C.byref(c), 4, 2, None)) == -1
    assert many(4, [3, -1]) == -1 and many(4, [0, 0, 0]) == -1
    # monotone in every count
    sizes = (0, 1, 2, 31, 32, 33, 255, 256, 257, 1000)
    for T in (1, 7):
        for g in range(3):
            prev = -1
            for B in sizes:
                counts = [40, 40, 40]
                counts[g] = B
                v = many(T, counts)
                assert v > prev and v % 16 == 0
                prev = v


def test_host_only_refusals_in_their_order():
    """In the order of include/rdv.h: the arguments, by name, before the handles are looked at — no GPU needed.  With invalid handles
    counts_host is read for one member."""
    lib = N.lib()
    keep = np.zeros(64, np.float32)
    p = keep.ctypes.data
    ws = (C.c_char * 64)()
    wsp = (C.addressof(ws) + 15) & ~15
    four = counts_of([4])

    def call(rows=None, out=None, counts=four, workspace=wsp, eps=0.2, ent=0.0, vf=0.5, **fields):
        r = N.LstmPpoRows(p, p, p, p, p, p, p, p, p, p, p, 4, 2, 4) if rows is None else rows
        o = N.LstmPpoSetOut(p, p, p, None, None) if out is None else out
        for k, v in fields.items():
            setattr(r if hasattr(r, k) else o, k, v)
        rc = lib.rdv_lstm_ppo_set_loss_grad(None, None, C.byref(r), counts, eps, ent, vf, workspace, 64, C.byref(o), None)
        return rc, lib.rdv_last_error().decode()

    rc = lib.rdv_lstm_ppo_set_loss_grad(None, None, None, four, 0.2, 0.0, 0.5, wsp, 64, None, None)
    assert rc == -1 and "rows is null" in lib.rdv_last_error().decode()
    r = N.LstmPpoRows(p, p, p, p, p, p, p, p, p, p, p, 4, 2, 4)
    rc = lib.rdv_lstm_ppo_set_loss_grad(None, None, C.byref(r), four, 0.2, 0.0, 0.5, wsp, 64, None, None)
    assert rc == -1 and "out is null" in lib.rdv_last_error().decode()
    rc, msg = call(counts=None)
    assert rc == -1 and "counts_host is null" in msg
    for name in ("obs", "actions", "old_log_prob", "advantages", "returns", "done", "actor_h0", "actor_c0", "critic_h0", "critic_c0", "envs"):
        rc, msg = call(**{name: None})
        assert rc == -1 and f"rows->{name} is null" in msg, msg
    for name in ("actor_grad", "critic_grad", "scalars"):
        rc, msg = call(**{name: None})
        assert rc == -1 and f"out->{name} is null" in msg, msg
    rc, msg = call(workspace=None)
    assert rc == -1 and "workspace is null" in msg
    # the counts are judged ahead of the sizes: a negative count, none positive, n_seq against their sum
    rc, msg = call(counts=counts_of([-4]), n_envs=0)
    assert rc == -1 and "counts_host[0] = -4 is negative" in msg, msg
    rc, msg = call(counts=counts_of([0]), n_envs=0)
    assert rc == -1 and "no positive count" in msg, msg
    rc, msg = call(n_seq=5, n_envs=0)
    assert rc == -1 and "rows->n_seq = 5" in msg and "sums to 4" in msg, msg
    for name in ("n_envs", "n_steps"):
        for v in (0, -3):
            rc, msg = call(**{name: v})
            assert rc == -1 and f"rows->{name}" in msg, msg
    big = (1 << 31) + 1
    rc, msg = call(counts=counts_of([big]), n_seq=big, n_steps=1)
    assert rc == -1 and "2^31" in msg, msg
    rc, msg = call(counts=counts_of([1 << 12]), n_seq=1 << 12, n_steps=1 << 20, workspace=wsp + 4)
    assert rc == -1 and "2^31" in msg, msg                       # more than 2^31 rows in a member, ahead of the alignment
    rc, msg = call(workspace=wsp + 4)
    assert rc == -1 and "16-byte aligned" in msg
    for kw, word in ((dict(eps=0.0), "clip_range"), (dict(eps=float("nan")), "clip_range"), (dict(ent=-1.0), "ent_coef"), (dict(vf=float("inf")), "vf_coef")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, msg
    rc, msg = call()
    assert rc == -5, (rc, msg)                                   # then the handles: RDV_ERR_BAD_HANDLE


# ------------------------------------------------------------------------------------------------------------ Python
def small_set(backend="torch"):
    case = S.make_set_case(32, (32,), (16,), "tanh", "hot", (256, 256, 40), 3, "random")
    return case, LstmPolicySet(S.make_members(case), list(case["sizes"]), backend=backend), S.make_buf(case)


def test_sequence_set_minibatches():
    assert "ppo_sequence_set_minibatches" in pkg.__all__ and pkg.ppo_sequence_set_minibatches is ppo.ppo_sequence_set_minibatches
    case, lset, _ = small_set()
    steps = ppo.ppo_sequence_set_minibatches(lset, 100, torch.Generator().manual_seed(4))
    assert len(steps) == 3 and all(len(step) == 3 for step in steps)
    assert [[None if p is None else int(p.numel()) for p in step] for step in steps] == [[100, 100, 40], [100, 100, None], [56, 56, None]]
    for g, sl in enumerate(lset.group_slices):
        mine = [step[g] for step in steps if step[g] is not None]
        assert sorted(torch.cat(mine).tolist()) == list(range(sl.start, sl.stop))            # every column exactly once, inside the slice
        assert all(p.dtype == torch.int64 and p.dim() == 1 and p._rdv_ppo_seq_set == (lset.num_rows, sl.start, sl.stop) for p in mine)
    again = ppo.ppo_sequence_set_minibatches(lset, 100, torch.Generator().manual_seed(4))
    assert all((a is None and b is None) or torch.equal(a, b) for x, y in zip(steps, again) for a, b in zip(x, y))
    with pytest.raises(ValueError):
        ppo.ppo_sequence_set_minibatches(lset, 0)


@pytest.mark.parametrize("normalize", [True, False])
def test_the_fallback_equals_the_members_own_call(normalize):
    case, lset, buf = small_set()
    pieces = S.pieces_of(case, (33, None, 1), duplicate=0)
    res = lset.ppo_sequence_grads(buf, pieces, normalize_advantage=normalize, **COEFS)
    assert len(res) == 3 and res[1] is None
    got = {g: [p.grad.clone() for group in ppo._sequence_params(lset[g]) for p in group] for g in (0, 2)}
    assert all(p.grad is None for group in ppo._sequence_params(lset[1]) for p in group)       # the absent member's parameters are not touched
    twins = S.make_members(case)
    for g in (0, 2):
        twins[g].backend = "torch"
        want = twins[g].ppo_sequence_grad(buf, pieces[g], normalize_advantage=normalize, **COEFS)
        for a, b in zip(got[g], [p.grad for group in ppo._sequence_params(twins[g]) for p in group]):
            assert torch.equal(a, b)
        for k in ppo.SCALAR_NAMES + ("log_prob", "values"):
            assert torch.equal(res[g][k], want[k]), (g, k)
        assert res[g]["log_prob"].shape == (case["T"], pieces[g].numel())


def test_checks_of_the_python_call():
    case, lset, buf = small_set()
    ok = S.pieces_of(case, (2, 2, 2))
    with pytest.raises(TypeError):
        ppo.ppo_sequence_set_grads(lset[0], buf, ok)
    with pytest.raises(TypeError):                                                   # the single-policy call keeps refusing a set
        ppo.ppo_sequence_grad(lset, buf)
    with pytest.raises(TypeError):                                                   # and so does the feed-forward set call
        lset.ppo_grads(buf, ok)
    assert not hasattr(lset, "adam_step")
    with pytest.raises(ValueError, match="one per member"):
        lset.ppo_sequence_grads(buf, ok[:2])
    with pytest.raises(ValueError, match="None"):
        lset.ppo_sequence_grads(buf, [None, None, None])
    with pytest.raises(ValueError, match=r"pieces\[1\]"):
        lset.ppo_sequence_grads(buf, [ok[0], ok[1].to(torch.int32), ok[2]])
    with pytest.raises(ValueError, match="clip_range"):
        lset.ppo_sequence_grads(buf, ok, clip_range=0.0)
    with pytest.raises(IndexError, match=r"pieces\[2\] span"):
        lset.ppo_sequence_grads(buf, [ok[0], ok[1], torch.tensor([512, 552])])
    with pytest.raises(IndexError, match=r"pieces\[1\] reach env columns \[255, 300\], member 1 owns 256\.\.511"):
        lset.ppo_sequence_grads(buf, [ok[0], torch.tensor([300, 255]), ok[2]])       # a piece that reaches the neighbour's columns
    with pytest.raises(ValueError, match="done"):
        lset.ppo_sequence_grads({k: v for k, v in buf.items() if k != "done"}, ok)
    with pytest.raises(ValueError, match="lstm_critic_state0"):
        lset.ppo_sequence_grads({k: v for k, v in buf.items() if k != "lstm_critic_state0"}, ok)
    narrow = {k: (v[:, :512].contiguous() if k not in ("lstm_state0", "lstm_critic_state0") else tuple(x[:512].contiguous() for x in v)) for k, v in buf.items()}
    with pytest.raises(ValueError, match="N must be the set's rows"):
        lset.ppo_sequence_grads(narrow, ok)
    # the mark of the minibatch helper lets a piece through unchecked; check=False does the same
    marked = torch.tensor([300, 255])
    marked._rdv_ppo_seq_set = (lset.num_rows, 256, 512)
    lset.ppo_sequence_grads(buf, [None, marked, None])
    lset.ppo_sequence_grads(buf, [None, torch.tensor([300, 255]), None], check=False)

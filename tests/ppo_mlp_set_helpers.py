"""
What the tests of the general set form (rdv_ppo_mlp_set_loss_grad) share: the spec pairs, the members of a
set of one pair, the rows, and (``flat``) tests/ppo_adam_reference.py's flat layout of a net.

Members: dense random nets of tests/ppo_mlp_reference.py (``nets``), seed 5 + 2 g for member g, so a wrong member's block cannot pass by
accident.  Rows: the 1,200 rows of ``ppo_mlp_reference.make_case`` for the pair (drawn for member 0; the comparisons are by equality of
bits with stand-alone calls on the same rows, so no condition on the ratios is needed), seen as T = 1, N = 1200 with the set sizes of
tests/test_ppo_set_grad.py.
"""
import numpy as np
import torch

import policy_mlp_reference as M
import ppo_mlp_reference as Q
import ppo_reference as P
from ppo_adam_reference import flat  # noqa: F401  (H.flat: the flat layout of rdv_ppo_mlp_grad_floats)
from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd.policy import ACTIVATIONS, MlpPolicy, PolicySet

SIZES = [256, 512, 432]
STARTS = [0, 256, 768]
# (pi, vf, activation): (a) the reference's custom pair; (b) an actor of 128-row workgroups beside a critic of 256-row ones; (c) the
# largest block; (d) the smallest widths
PAIRS = {"a": ((32, 32), (32, 32), "relu"), "b": ((64, 64, 64), (16,), "tanh"), "c": ((64, 64, 64, 64), (64, 64, 64, 64), "tanh"),
         "d": ((16, 16), (16, 16), "sigmoid")}


def specs(pair):
    pi, vf, act = pair
    return N.MlpSpec.make(list(pi), ACTIVATIONS[act][0]), N.MlpSpec.make(list(vf), ACTIVATIONS[act][0])


def member_nets(pair, members=3):
    pi, vf, act = pair
    return [Q.nets(pi, vf, act, seed=5 + 2 * g) for g in range(members)]


def policy_of(nets, **kw):
    return MlpPolicy(M.weights_dict(*nets), activation_fn=nets[0]["act"], **kw)


def make_set(pair, members=3, sizes=None, **kw):
    return PolicySet([policy_of(n) for n in member_nets(pair, members)], SIZES if sizes is None else sizes, **kw)


def columns(pair):
    """The five columns [1200, ...] (numpy, read-only) of the pair's case."""
    case = Q.make_case(*pair)
    return {k: case[k] for k in P.COLUMNS}


def make_buf(cols):
    """numpy or torch columns as the [1, 1200, ...] columns of a rollout"""
    out = {}
    for k, v in cols.items():
        t = torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else v
        out["log_prob" if k == "old_log_prob" else k] = t.reshape(1, P.ROWS, *t.shape[1:])
    return out


def member_indices(g, n, seed=4):
    """n shuffled rows of member g's env columns (T = 1), one of them twice (tests/test_ppo_set_grad.py)"""
    rng = np.random.default_rng([seed, g, n])
    idx = STARTS[g] + rng.permutation(SIZES[g])[:n].astype(np.int64)
    if n >= 4:
        idx[n // 2] = idx[1]
    return torch.from_numpy(idx)


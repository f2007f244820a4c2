"""
The output bits of the three PPO gradient entry points (rdv_ppo_loss_grad, rdv_ppo_mlp_loss_grad, rdv_ppo_set_loss_grad) as sha256
digests, for tests/test_gpu_ppo_digests.py and tests/golden/make_golden_ppo_digests.py: ``digests()`` runs every case on the library that
``_native`` loads and returns {case id: {output name: sha256 of the tensor's raw bytes}} for actor_grad, critic_grad, scalars, log_prob
and values.  The kernels are deterministic (no floating-point atomic, waves in wave order, workgroups in index order), so a build that
keeps every operation in its order keeps every digest.

Inputs are the NumPy cases the other PPO tests use, with their fixed seeds (ppo_reference.make_case, ppo_mlp_reference.make_case,
test_ppo_set_grad.set_columns); the calls are theirs too.  The cases are the smallest at which each piece the two kernel units share can
go wrong:
  * shipped call, n = 1 (one row, seven waves without rows), 33 (a second wave of one row), 257 (two workgroups: the last kernel adds
    rows) and 549, each with rows in order (the contiguous gather) and through an index vector (the indexed gather); the rows' ratios lie
    on both sides of the clip range and inside it, where the two surrogate terms tie; and n = 549 with one NaN advantage and with one NaN
    old_log_prob (ppo_reference.with_nan), whose bytes — NaN payloads included — go through the loss terms' NaN path;
  * general call, four pairs that reach all six (tiles, k-steps) shapes of the backward switch, both widths of the layer-0 step and both
    wave counts, at n = 1, 33 and 257 in order and at the largest n through an index vector; the pair whose critic has four waves per
    workgroup (4 x 64) also at n = 129, its two workgroups;
  * set call, three members with counts (33, 0, 257): the outputs of the member without samples keep the NaNs they were filled with, and
    those bytes are part of the digest.
"""
import hashlib

import torch

import ppo_mlp_reference as Q
import ppo_reference as P

SHIPPED_MEMBER = "random"
SHIPPED_SHAPES = (1, 33, 257, 549)
NAN_COLUMNS = ("advantages", "old_log_prob")         # one NaN in row 540 of n = 549: the NaN path of the loss terms, bit for bit
MLP_PAIRS = (((16,), (16,), "sigmoid"), ((32, 32), (32, 32), "relu"), ((16, 64), (64, 64, 64, 64), "tanh"), ((64, 16, 32), (32, 64, 16), "relu"))
MLP_SHAPES = (1, 33, 257)
FOUR_WAVE_SHAPE = 129
SET_COUNTS = (33, 0, 257)
OUTPUTS = ("actor_grad", "critic_grad", "scalars", "log_prob", "values")


def sha(tensors):
    torch.cuda.synchronize()
    return {name: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for name, t in zip(OUTPUTS, tensors)}


def mlp_shapes(pair):
    """(n, indexed) of one pair: every shape in order, the largest through an index vector too"""
    ns = MLP_SHAPES + ((FOUR_WAVE_SHAPE,) if any(len(a) == 4 and min(a) == 64 for a in pair[:2]) else ())
    return [(n, False) for n in sorted(ns)] + [(max(ns), True)]


def digests():
    import test_gpu_ppo_grad as G
    import test_gpu_ppo_mlp_grad as GM
    import test_gpu_ppo_set_grad as GS
    import test_ppo_set_grad as S

    out = {}
    case = P.make_case(SHIPPED_MEMBER)
    pol, cols = G.make_policy(case["actor"], case["critic"]), G.device_columns(case)
    for n in SHIPPED_SHAPES:
        for indexed in (False, True):
            out[f"shipped-{n}-{'indexed' if indexed else 'ordered'}"] = sha(G.call(pol, cols, n, P.index_vector(n) if indexed else None)["raw"])
    for column in NAN_COLUMNS:
        out[f"shipped-{P.DEAD_N}-nan-{column}"] = sha(G.call(pol, G.device_columns(P.with_nan(case, column)), P.DEAD_N)["raw"])
    pol.close()

    for pair in MLP_PAIRS:
        case = Q.make_case(*pair)
        nets = (case["actor"], case["critic"])
        pol, cols = GM.make_policy(*nets), GM.device_columns(case)
        for n, indexed in mlp_shapes(pair):
            out[f"{Q.case_id(pair)}-{n}-{'indexed' if indexed else 'ordered'}"] = sha(GM.call(pol, nets, cols, n, P.index_vector(n) if indexed else None)["raw"])
        pol.close()

    pset = S.make_set().to(GS.DEV)
    cols = {k: torch.from_numpy(v.copy()).to(GS.DEV) for k, v in S.set_columns().items()}
    out["set-" + "-".join(map(str, SET_COUNTS))] = sha(GS.set_call(pset, cols, list(SET_COUNTS), GS.index_vectors(SET_COUNTS)))
    pset.close()
    return out

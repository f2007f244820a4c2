"""
The bits that the two optimiser entry points (rdv_ppo_set_adam_step, rdv_ppo_mlp_set_adam_step; csrc/rdv_ppo_adam.h) leave behind, as
sha256 digests, for tests/test_gpu_ppo_adam_digests.py and tests/golden/make_golden_ppo_adam_digests.py: ``digests()`` runs every case on
the library that ``_native`` loads and returns {"<case>/<call>": {array: sha256 of its raw bytes}} — after EACH call the eight
RdvAdamState arrays (``coef`` rows of skipped members included) and every member's actor and critic block, masked and skipped members
too: their bytes must be the earlier ones.  The other tests hold p, m, v to the float32 restatement and the blocks to the host packer, but
``coef`` and exp(log_std) only to 1 ulp; the kernels are deterministic (double sums in a fixed order, no atomic), so a build that keeps
every operation in its order keeps every digest.

The cases are the smallest at which each piece the two calls share is reached on each of its paths; rigs, members and gradients are those
of tests/test_gpu_ppo_adam.py and tests/test_gpu_ppo_mlp_set_adam.py, with their fixed seeds:
  * shipped call: P = 1 on plain handles, P = 3 with member 1 masked out of the first three steps, and P = 64 (the cap: the mask has no
    bit to spare), each taking the four GRAD_CASES as consecutive steps (zero, clipped, unclipped, max_grad_norm = inf); one step on the
    corner members (the shift rule's branches, fp16 subnormals and rounding corners); a warm step and then one with a NaN gradient in
    one member and an infinite one in another (the skip path);
  * general call, three members each: pairs a (32-wide: zero fragments for the missing rows and k-steps), b (three layers beside one:
    different depths per net), c (4 x 64: the largest LDS copy), d (16-wide) of ppo_mlp_set_helpers.PAIRS, and the [16, 64] pair with
    the corners "cross", "big", "tiny" in its 64-wide layer; the four GRAD_CASES as consecutive steps, member 1 masked out of the second,
    then one step with a NaN in member 0's gradient;
  * forwarding: one step of a default-spec set through rdv_ppo_mlp_set_adam_step and, from the same weights and gradients, through
    rdv_ppo_set_adam_step (FORWARD_CASES: the two must agree, and both are in the fixture).
"""
import ctypes as C
import hashlib

import numpy as np
import torch

import ppo_adam_reference as A
import ppo_mlp_set_helpers as H
from reinforcement_learning_rendezvous_amd import _native as N

SHIPPED_CONFIGS = {"P1-plain": 1, "P3-member1-masked": 3, "P64": 64}
MLP_PAIRS = {**{k: H.PAIRS[k] for k in "abcd"}, "16x64-corners": ((16, 64), (16, 64), "tanh")}
FORWARD_CASES = ("forward/rdv_ppo_mlp_set_adam_step", "forward/rdv_ppo_set_adam_step")


def sha(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def digest(read):
    """{array: sha256} of one read: the eight state arrays and [(actor block, critic block)] per member"""
    out = {name: sha(read[name]) for name, _ in N.AdamState._fields_}
    for g, pair in enumerate(read["blocks"]):
        out.update({f"{net}_block[{g}]": sha(b) for net, b in zip(("actor", "critic"), pair)})
    return out


def shipped_cases(out):
    import test_gpu_ppo_adam as T

    def run(case, rig, calls):
        """calls: [(call id, gradients per member, keyword arguments of Rig.step)]"""
        try:
            for name, grads, kw in calls:
                rig.set_grads(grads)
                N.check(rig.step(**kw))
                out[f"{case}/{name}"] = digest(rig.read())
        finally:
            rig.close()

    for config, P in SHIPPED_CONFIGS.items():
        live = lambda k: [0, 2] if config == "P3-member1-masked" and k < 3 else list(range(P))
        run(f"shipped-{config}", T.Rig(T.members(P), plain=config == "P1-plain"),
            [(f"{k}-{name}", T.case_grads(P, name, scale, seed=k), dict(mask=sum(1 << g for g in live(k)), max_norm=max_norm))
             for k, (name, scale, max_norm) in enumerate(A.GRAD_CASES)])
    rig, _, grads = T.corner_rig()
    run("shipped-corners", rig, [("0-clipped", grads, {})])
    bad = [list(g) for g in T.case_grads(3, "unclipped", 0.2, seed=2)]
    bad[0][1][5000] = np.float32("nan")
    bad[1][0][17] = np.float32("-inf")
    run("shipped-nonfinite", T.Rig(T.members(3, seed=60)), [("0-warm", T.case_grads(3, "clipped", 3.0, seed=1), {}), ("1-nan-inf", [tuple(g) for g in bad], {})])
    for call in FORWARD_CASES:
        run("forward", T.Rig(T.members(3, seed=70)), [(call.split("/")[1], T.case_grads(3, "clipped", 3.0, seed=4), dict(mask=5, call=call.split("/")[1]))])


def mlp_cases(out):
    import test_gpu_ppo_mlp_set_adam as TM
    from reinforcement_learning_rendezvous_amd.policy import PolicySet

    for key, pair in MLP_PAIRS.items():
        if key in H.PAIRS:
            pset = H.make_set(pair).to(TM.DEV)
        else:
            pset = PolicySet([H.policy_of(TM.corner(n, which, 1)) for n, which in zip(H.member_nets(pair), A.CORNERS)], H.SIZES).to(TM.DEV)
        try:
            st, ad = TM.ready(pset, TM.columns(pair))
            ga, gc = int(st["actor"].shape[1]), int(st["critic"].shape[1])
            calls = [(f"{k}-{name}", [A.gradients(10 * k + g, scale, ga, gc) for g in range(3)], 0b101 if k == 1 else 0b111, max_norm)
                     for k, (name, scale, max_norm) in enumerate(A.GRAD_CASES)]
            nan = [list(A.gradients(40 + g, 0.2, ga, gc)) for g in range(3)]
            nan[0][0][17] = np.float32("nan")
            calls.append(("4-nan", nan, 0b111, 0.5))
            for name, grads, mask, max_norm in calls:
                st["actor"].copy_(torch.from_numpy(np.stack([g[0] for g in grads])))
                st["critic"].copy_(torch.from_numpy(np.stack([g[1] for g in grads])))
                N.check(N.lib().rdv_ppo_mlp_set_adam_step(pset._hip_handle(TM.DEV), pset._critic_handle(TM.DEV), C.byref(ad["c"]), C.c_void_p(st["actor"].data_ptr()),
                                                          C.c_void_p(st["critic"].data_ptr()), C.c_uint64(mask), TM.LR, TM.B1, TM.B2, TM.EPS, max_norm,
                                                          C.c_void_p(torch.cuda.current_stream(TM.DEV).cuda_stream)))
                torch.cuda.synchronize()
                out[f"mlp-{key}/{name}"] = digest(TM.snapshot(pset, ad))
        finally:
            pset.close()


def digests():
    out = {}
    shipped_cases(out)
    mlp_cases(out)
    return out

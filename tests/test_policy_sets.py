"""
CPU-side checks of policy sets (include/rdv.h: one batch, several actors and critics, one launch): the constructor's refusals, the
PyTorch fallback of PolicySet.act / value / advantages against the members' own modules and tests/advantages_reference.py, the resource
report of the new translation unit, and the instruction streams of the existing actor / critic / rollout kernels against the table of
profiles/policy_sets_isa_diff.md.  No GPU needed.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import advantages_reference as AR
import policy_mlp_reference as M
from reinforcement_learning_rendezvous_amd import _native as N

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256, 512, 200]


def _weights(arch, act, g, critic=True):
    net = M.dense(list(arch), act, seed=40 + g)
    net["log_std"] = np.random.default_rng(900 + g).uniform(-1.4, -0.4, 6).astype(np.float32)
    return M.weights_dict(net, M.critic_of(M.dense(list(arch), act, seed=70 + g)) if critic else None)


def _members(arch=(32, 16), act="relu", count=3, no_critic=()):
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    return [MlpPolicy(_weights(arch, act, g, critic=g not in no_critic), net_arch=list(arch), activation_fn=act) for g in range(count)]


def _set(**kw):
    from reinforcement_learning_rendezvous_amd import PolicySet
    return PolicySet(_members(**kw), SIZES)


# ---------------------------------------------------------------------------------------------------------------- constructor
def test_members_of_another_architecture_or_activation_are_refused_naming_the_member():
    from reinforcement_learning_rendezvous_amd import PolicySet
    a = _members()
    with pytest.raises(ValueError, match=r"member 2 has pi_arch = \[64, 64\], member 0 has \[32, 16\]"):
        PolicySet(a[:2] + _members(arch=(64, 64), count=1), SIZES)
    with pytest.raises(ValueError, match="member 1 has activation = 'tanh', member 0 has 'relu'"):
        PolicySet([a[0]] + _members(act="tanh", count=1) + [a[2]], SIZES)
    with pytest.raises(TypeError, match="member 1 is a Linear"):
        PolicySet([a[0], torch.nn.Linear(17, 6), a[2]], SIZES)
    with pytest.raises(ValueError, match="at least one member"):
        PolicySet([], [])


@pytest.mark.parametrize("sizes,rows,words", [
    ([200, 512, 256], None, "group 0 has size 200: every group but the last must be a multiple of 256"),
    ([256, 0, 712], None, "group 1 has size 0: sizes must be positive"),
    ([256, 512, 200], 1000, "group 2 (the last) ends at env 968, the batch has 1000 envs"),
    ([256, 512, 456], 968, "group 2 ends at env 1224, the batch has 968 envs"),
])
def test_group_sizes_obey_the_rule_of_parameter_groups(sizes, rows, words):
    """the messages are rdv_param_groups_check's: the library gives the same words for the same layout"""
    from reinforcement_learning_rendezvous_amd import PolicySet
    with pytest.raises(ValueError) as e:
        PolicySet(_members(), sizes, num_rows=rows)
    assert words in str(e.value) and str(e.value).startswith("rdv_param_groups_check:")
    import ctypes as C
    n = sum(sizes) if rows is None else rows
    assert N.lib().rdv_param_groups_check(n, len(sizes), (C.c_int64 * len(sizes))(*sizes)) == -1
    assert N.lib().rdv_last_error().decode() == str(e.value)


def test_length_mismatches_are_refused():
    from reinforcement_learning_rendezvous_amd import PolicySet
    with pytest.raises(ValueError, match="3 policies but 2 group sizes"):
        PolicySet(_members(), [256, 712])
    s = _set()
    with pytest.raises(ValueError, match="a list of 3 dicts"):
        s.update_weights(weights=[None, None])
    with pytest.raises(IndexError, match="member 3 of 3"):
        s.update_weights(member=3)
    with pytest.raises(ValueError, match="100 rows, the policy set owns 968"):
        s.act(torch.zeros(100, 17))
    with pytest.raises(ValueError, match="100 rows, the policy set owns 968"):
        s.value(torch.zeros(2, 100, 17))


def test_members_slices_and_noise_state():
    s = _set()
    assert len(s) == 3 and s[1] is s.policies[1] and [(x.start, x.stop) for x in s.group_slices] == [(0, 256), (256, 768), (768, 968)]
    assert s.num_rows == 968 and s._calls == 0 and s.noise_seed == s[0].noise_seed and s.has_critic
    assert s.pi_arch == [32, 16] and s.vf_arch == [32, 16] and s.activation == "relu" and not s.shipped_arch
    s.close()                                     # no handle was made: nothing to free, no library call


def test_a_member_without_a_critic_makes_the_set_criticless():
    s = _set(no_critic=(1,))
    assert [p.has_critic for p in s] == [True, False, True] and not s.has_critic
    ro = dict(obs=torch.zeros(2, 968, 17), reward=torch.zeros(2, 968), done=torch.zeros(2, 968, dtype=torch.uint8), last_obs=torch.zeros(968, 17))
    with pytest.raises(ValueError, match="no critic") as e:
        s.advantages(ro)
    with pytest.raises(ValueError) as single:
        s[1].advantages(ro)
    assert str(e.value) == str(single.value)      # as MlpPolicy.advantages does


# ---------------------------------------------------------------------------------------------------------------- CPU fallback
@pytest.mark.parametrize("arch,act", [((64, 64), "tanh"), ((32, 16), "relu")], ids=["64x64-tanh", "32x16-relu"])
def test_cpu_fallback_equals_the_members_on_their_slices(arch, act):
    s = _set(arch=arch, act=act)
    rng = np.random.default_rng(3)
    obs = torch.from_numpy(rng.uniform(-1, 1, (968, 17)).astype(np.float32))
    got = s.act(obs, deterministic=True)
    assert got.shape == (968, 6)
    for p, sl in zip(s, s.group_slices):
        assert torch.equal(got[sl], p.act(obs[sl], deterministic=True))
    assert not torch.equal(s[0].act(obs[:8]), s[1].act(obs[:8]))                 # the members differ
    out = torch.empty(968, 6)
    assert s.act(obs, out=out) is out and torch.equal(out, got)
    obs3 = torch.from_numpy(rng.uniform(-1, 1, (3, 968, 17)).astype(np.float32))
    v = s.value(obs3)
    assert v.shape == (3, 968)
    for p, sl in zip(s, s.group_slices):
        assert torch.equal(v[:, sl], p.value(obs3[:, sl, :]))
    # advantages: the members' values, then tests/advantages_reference.py per member
    T = 5
    ro = dict(obs=torch.from_numpy(rng.uniform(-1, 1, (T, 968, 17)).astype(np.float32)),
              reward=torch.from_numpy(rng.normal(0, 1, (T, 968)).astype(np.float32)),
              done=torch.from_numpy((rng.uniform(0, 1, (T, 968)) < 0.2).astype(np.uint8)),
              last_obs=torch.from_numpy(rng.uniform(-1, 1, (968, 17)).astype(np.float32)))
    res = s.advantages(dict(ro), gamma=0.99, gae_lambda=0.95)
    for p, sl in zip(s, s.group_slices):
        values, last = p.value(ro["obs"][:, sl, :]), p.value(ro["last_obs"][sl])
        assert torch.equal(res["values"][:, sl], values) and torch.equal(res["last_value"][sl], last)
        adv, ret = AR.gae32(ro["reward"][:, sl].numpy(), ro["done"][:, sl].numpy(), values.numpy(), last.numpy(), 0.99, 0.95)
        np.testing.assert_array_equal(res["advantages"][:, sl].numpy(), adv)
        np.testing.assert_array_equal(res["returns"][:, sl].numpy(), ret)
    again = s.advantages(dict(ro), out=res)                                        # the buffers are reused
    assert all(again[k] is res[k] for k in ("values", "last_value", "advantages", "returns"))
    # update_weights without a live handle: the member module takes the dict, the others stay
    new = _weights(arch, act, 9)
    before0 = s[0].l1.weight.clone()
    s.update_weights(member=1, weights=new)
    np.testing.assert_array_equal(s[1].l1.weight.numpy(), new["mlp_extractor.policy_net.0.weight"])
    assert torch.equal(s[0].l1.weight, before0)


# ---------------------------------------------------------------------------------------------------------------- the build
SET_KERNELS = ["policy_set_act_kernel", "policy_set_value_kernel"] + [f"mlp_set_kernelILi{a}ELb{c}EE" for a in (0, 1, 2) for c in (0, 1)]


def test_resource_report_of_the_new_translation_unit():
    """hipcc's kernel-resource remarks for csrc/rdv_policy_sets.hip alone (gfx950 cross-compile, the Makefile's flags): all eight set
    kernels, each without scratch and within 128 VGPRs (two workgroups per CU for the shipped block, four waves per SIMD as mlp_kernel
    asks)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_diff as K
    hipcc, flags = K.hipflags(N.CSRC)
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "rdv_policy_sets.hip"], cwd=N.CSRC,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    vgprs, scratch, name = {}, {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert len(vgprs) == 8 and set(vgprs) == set(scratch), sorted(vgprs)
    for w in SET_KERNELS:
        hits = [k for k in vgprs if w in k]
        assert len(hits) == 1, (w, sorted(vgprs))
        assert scratch[hits[0]] == 0 and vgprs[hits[0]] <= 128, (w, scratch[hits[0]], vgprs[hits[0]])
    make = open(os.path.join(N.CSRC, "Makefile")).read()       # and `make resource` (tests/test_abi.py: no scratch anywhere) covers the unit
    assert re.search(r"kernel-resource-usage -c -o /dev/null rdv_policy_sets\.hip", make)


def test_existing_actor_critic_and_rollout_kernels_are_what_they_were():
    """profiles/policy_sets_isa_diff.md records, for policy_act_kernel, policy_value_kernel, the six mlp_kernels and both
    rollout_kernels, that the parent's and this tree's gfx950 instruction streams are identical, with a digest of each stream.  This
    tree's rdv_hip.hip and rdv_policy_mlp.hip, compiled again, still give those digests: a header that perturbs them is moved.  Rows
    marked `changed` there hold the digest of a kernel as a later change left it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_diff as K
    rows = re.findall(r"^\| (\w+): `([^`]+)` \| (\d+) \| (\d+) \| `(\w+)` \| (\w+) \|$", open(os.path.join(ROOT, "profiles", "policy_sets_isa_diff.md")).read(), re.M)
    # (the two rollout kernels were changed on purpose later — the order of their statistics sums — and are recorded as they are now)
    assert len(rows) == 10 and all((r[5] == "yes" and r[2] == r[3]) or (r[5] == "changed" and "rollout_kernel" in r[1]) for r in rows), rows
    assert sum(r[5] == "changed" for r in rows) == 2
    assert sorted(r[1].split("::")[1].split("<")[0] for r in rows) == ["mlp_kernel"] * 6 + ["policy_act_kernel", "policy_value_kernel"] + ["rollout_kernel"] * 2
    for unit in ("rdv_hip", "rdv_policy_mlp"):
        got = K.streams(unit)
        for _, name, _, count, sha, _ in [r for r in rows if r[0] == unit]:
            assert name in got, (name, sorted(got))
            assert (len(got[name]), K.digest(got[name])) == (int(count), sha), name

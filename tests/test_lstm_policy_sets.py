"""
CPU-side checks of recurrent policy sets (include/rdv.h, "Recurrent policy sets"): the PyTorch fallback of LstmPolicySet against its
members stand-alone, the Python and C refusals that need no GPU, the pins that stay (PolicySet refuses an LstmPolicy; more layers and a
shared LSTM are refused), the resource report of the set forms of the kernels, and the instruction streams of the tree's recurrent
kernels against the table of profiles/lstm_sets_isa_diff.md.  No GPU needed.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import advantages_reference as AR
import policy_lstm_reference as L
import policy_reference as R
from reinforcement_learning_rendezvous_amd import _native as N

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256, 37]


def _weights(H, g, arch=(64, 64), act="tanh"):
    net = L.hot(H, arch, act, seed=51 + g)
    net = dict(net, log_std=np.random.default_rng(900 + g).uniform(-1.4, -0.4, 6).astype(np.float32))
    return L.weights_dict(net, L.critic_of(L.default_init(H, arch, act, seed=77 + g)))


def _member(H=32, g=0, arch=(64, 64), act="tanh", **kw):
    from reinforcement_learning_rendezvous_amd import LstmPolicy
    return LstmPolicy(_weights(H, g, arch, act), activation_fn=act, backend="torch", **kw)


def _set(H=32, sizes=SIZES, **kw):
    from reinforcement_learning_rendezvous_amd import LstmPolicySet
    return LstmPolicySet([_member(H, g) for g in range(len(sizes))], sizes, backend="torch", **kw)


# ---------------------------------------------------------------------------------------------------------------- the class
def test_the_class_is_exported_and_holds_its_members():
    import reinforcement_learning_rendezvous_amd as pkg
    assert "LstmPolicySet" in pkg.__all__ and pkg.LstmPolicySet is _set().__class__
    s = _set(seed=7)
    assert len(s) == 2 and s[1] is s.policies[1] and [(x.start, x.stop) for x in s.group_slices] == [(0, 256), (256, 293)]
    assert s.n_rows == 293 and s._calls == 0 and s.noise_seed == 7 and s.lstm_hidden_size == 32 and s._pending == {"l": True, "v": True}
    assert s.pi_arch == [64, 64] and s.vf_arch == [64, 64] and s.activation == "tanh"
    assert s._rows(293) == 293
    s.close()                                     # no handle was made: nothing to free, no library call


def test_cpu_fallback_equals_the_members_on_their_slices():
    """3 steps with episode starts: act, value and the state of the set against stand-alone policies of the members' weights on their
    slices; a non-committing value writes nothing; then advantages (a critic loop of its own plus float32 GAE), twice in a row."""
    H, n = 32, sum(SIZES)
    s = _set(H)
    twins = [_member(H, g, n_rows=m) for g, m in enumerate(SIZES)]
    obs, starts = L.obs_sequence(n, 4), L.episode_starts(n, 3)
    for t in range(3):
        o = torch.from_numpy(obs[t])
        a, v = s.act(o, episode_start=starts[t]), s.value(o, episode_start=starts[t])
        assert a.shape == (n, 6) and v.shape == (n,)
        for p, sl in zip(twins, s.group_slices):
            assert torch.equal(a[sl], p.act(o[sl], episode_start=starts[t][sl])) and torch.equal(v[sl], p.value(o[sl], episode_start=starts[t][sl]))
            for got, want in zip(s.state + s.critic_state, p.state + p.critic_state):
                assert torch.equal(got[sl], want)
    latent = torch.from_numpy(obs[3][:37, :1]).expand(37, H)                        # the members differ on one input
    assert not torch.equal(s[0]._trunk_torch("l", latent), s[1]._trunk_torch("l", latent))
    before = s.critic_state
    o = torch.from_numpy(obs[3])
    peek = s.value(o, commit=False)
    assert all(torch.equal(x, y) for x, y in zip(before, s.critic_state)) and s._pending["v"] is False
    assert torch.equal(peek, torch.cat([p.value(o[sl], commit=False) for p, sl in zip(twins, s.group_slices)]))
    out = torch.empty(n, 6)
    raw, lp = torch.empty(n, 6), torch.empty(n)
    assert s.act(o, out=out, raw_out=raw, log_prob_out=lp) is out
    for g, sl in enumerate(s.group_slices):                                          # deterministic log_prob: the member's own log_std
        assert torch.allclose(lp[sl], torch.full((sl.stop - sl.start,), -float(s[g].log_std.sum()) - 3.0 * float(np.log(2.0 * np.pi))))
    assert torch.equal(out, raw.clamp(-1.0, 1.0))
    # state set / get, reset_state(mask), state_at_start
    h, c = s.state
    s.state = (c, h)
    assert torch.equal(s.state[0], c) and torch.equal(s.state[1], h)
    mask = np.arange(n) % 4 == 1
    s.reset_state(mask)
    assert (s.state[0][mask] == 0).all() and torch.equal(s.state[0][~mask], c[~mask]) and (s.critic_state[1][mask] == 0).all()
    s._pending["l"] = torch.from_numpy(mask.astype(np.uint8))
    h0, _ = s.state_at_start("l")
    assert (h0[mask] == 0).all() and torch.equal(h0[~mask], s.state[0][~mask])
    with pytest.raises(ValueError, match="100 rows, the policy owns the state of 293"):
        s.act(torch.zeros(100, 17))
    # advantages
    T = 4
    rng = np.random.default_rng(5)
    s2 = _set(H)
    twins = [_member(H, g, n_rows=m) for g, m in enumerate(SIZES)]
    for call in range(2):
        ro = dict(obs=torch.from_numpy(L.obs_sequence(n, T, seed=70 + call)), reward=torch.from_numpy(rng.normal(size=(T, n)).astype(np.float32)),
                  done=torch.from_numpy((rng.random((T, n)) < 0.3).astype(np.uint8)), last_obs=torch.from_numpy(R.distinct_rows(n, seed=90 + call)))
        got = s2.advantages(dict(ro), gamma=0.98, gae_lambda=0.9)
        for p, sl in zip(twins, s2.group_slices):
            want = p.advantages({k: (v[:, sl] if k != "last_obs" else v[sl]).contiguous() for k, v in ro.items()}, gamma=0.98, gae_lambda=0.9)
            for col in ("values", "advantages", "returns"):
                np.testing.assert_array_equal(got[col][:, sl].numpy(), want[col].numpy(), err_msg=f"{col}, call {call}")
            np.testing.assert_array_equal(got["last_value"][sl].numpy(), want["last_value"].numpy())
        adv, ret = AR.gae32(ro["reward"].numpy(), ro["done"].numpy(), got["values"].numpy(), got["last_value"].numpy(), 0.98, 0.9)
        np.testing.assert_array_equal(got["advantages"].numpy(), adv)
        np.testing.assert_array_equal(got["returns"].numpy(), ret)
        assert torch.equal(s2._pending["v"], ro["done"][T - 1])
    # update_weights without a live handle: the member module takes the dict, the others stay
    new = _weights(H, 9)
    before0 = s2[0].lstm_actor.weight_hh_l0.clone()
    s2.update_weights(member=1, weights=new)
    np.testing.assert_array_equal(s2[1].lstm_actor.weight_hh_l0.numpy(), new["lstm_actor.weight_hh_l0"])
    assert torch.equal(s2[0].lstm_actor.weight_hh_l0, before0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals_by_name():
    from reinforcement_learning_rendezvous_amd import LstmPolicySet, MlpPolicy, PolicySet, LstmPolicy
    a, b = _member(32, 0), _member(32, 1)
    with pytest.raises(TypeError, match="member 1 is a MlpPolicy, not an LstmPolicy"):
        LstmPolicySet([a, MlpPolicy()], SIZES)
    with pytest.raises(ValueError, match="member 1 has lstm_hidden_size = 64, member 0 has 32"):
        LstmPolicySet([a, _member(64, 1)], SIZES)
    with pytest.raises(ValueError, match=r"member 1 has pi_arch = \[16\], member 0 has \[64, 64\]"):
        LstmPolicySet([a, LstmPolicy(lstm_hidden_size=32, net_arch=dict(pi=[16], vf=[64, 64]))], SIZES)
    with pytest.raises(ValueError, match=r"member 1 has vf_arch = \[16\], member 0 has \[64, 64\]"):
        LstmPolicySet([a, LstmPolicy(lstm_hidden_size=32, net_arch=dict(pi=[64, 64], vf=[16]))], SIZES)
    with pytest.raises(ValueError, match="member 1 has activation = 'relu', member 0 has 'tanh'"):
        LstmPolicySet([a, LstmPolicy(lstm_hidden_size=32, activation_fn="relu")], SIZES)
    with pytest.raises(ValueError, match="at least one member"):
        LstmPolicySet([], [])
    with pytest.raises(ValueError, match="2 policies but 3 group sizes"):
        LstmPolicySet([a, b], [256, 256, 37])
    for sizes, words in (([100, 256], "group 0 has size 100: every group but the last must be a multiple of 256"), ([256, 0], "group 1 has size 0: sizes must be positive")):
        with pytest.raises(ValueError) as e:
            LstmPolicySet([a, b], sizes)
        assert words in str(e.value) and str(e.value).startswith("rdv_param_groups_check:")
    s = LstmPolicySet([a, b], SIZES)
    with pytest.raises(IndexError, match="member 2 of 2"):
        s.update_weights(member=2)
    with pytest.raises(ValueError, match="a list of 2 dicts"):
        s.update_weights(weights=[None])
    # the pins that stay
    with pytest.raises(TypeError, match="not an MlpPolicy"):
        PolicySet([a], [8])
    with pytest.raises(ValueError, match="n_lstm_layers = 2"):
        LstmPolicy(n_lstm_layers=2)
    with pytest.raises(ValueError, match="shared_lstm"):
        LstmPolicy(shared_lstm=True)
    for kw, word in ((dict(n_layers=2), "n_layers = 2"), (dict(shared=1), "shared = 1")):
        spec = N.LstmSpec.make(64, [64, 64], **kw)
        assert N.lib().rdv_lstm_spec_check(C.byref(spec)) == -6 and word in N.lib().rdv_last_error().decode()


def _c_arrays(members, prefix="l"):
    """the arguments of rdv_lstm_policy_set_create behind the sizes, from LstmPolicy modules (kept alive by the returned list)"""
    from reinforcement_learning_rendezvous_amd.policy import _ptrs
    host = [p._host_arrays(prefix) for p in members]
    P = len(host)
    lstm = [_ptrs([m[0][k] for m in host]) for k in range(4)]
    wps, bps = [_ptrs(m[1]) for m in host], [_ptrs(m[2]) for m in host]
    wpp = (C.c_void_p * P)(*[C.addressof(a) for a in wps])
    bpp = (C.c_void_p * P)(*[C.addressof(a) for a in bps])
    lsp = _ptrs([m[3][0] for m in host]) if prefix == "l" else None
    return lstm, wpp, bpp, lsp, [host, wps, bps]


def test_create_refuses_before_any_device():
    """the order of work: the spec, the sizes, every member's arrays — all on the host, so all testable without a GPU (a call that got
    past them would fail at the device with another code)"""
    lib = N.lib()
    h = C.c_void_p()
    INVALID, BAD_PARAMS = -1, -6
    members = [_member(32, 0), _member(32, 1)]
    lstm, wpp, bpp, lsp, keep = _c_arrays(members)
    ok = N.LstmSpec.make(32, [64, 64])
    sizes = lambda *a: (C.c_int64 * len(a))(*a)
    msg = lambda: lib.rdv_last_error().decode()
    # the spec first: a bad spec is named even with null arrays
    bad = N.LstmSpec.make(100, [64, 64])
    assert lib.rdv_lstm_policy_set_create(C.byref(bad), 2, sizes(256, 37), *lstm, wpp, bpp, lsp, 0, C.byref(h)) == BAD_PARAMS and "hidden_size = 100" in msg()
    assert lib.rdv_lstm_critic_set_create(C.byref(N.LstmSpec.make(32, [64, 64], n_layers=2)), 2, sizes(256, 37), *lstm, wpp, bpp, 0, C.byref(h)) == BAD_PARAMS and "n_layers = 2" in msg()
    assert lib.rdv_lstm_policy_set_create(C.byref(N.LstmSpec.make(32, [64, 64], shared=1)), 2, sizes(256, 37), *lstm, wpp, bpp, lsp, 0, C.byref(h)) == BAD_PARAMS and "shared = 1" in msg()
    # n_members = 0
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 0, sizes(256), *lstm, wpp, bpp, lsp, 0, C.byref(h)) == INVALID and "n_members = 0" in msg()
    # the sizes, by the rule of parameter groups (the member is named as "group"), before the arrays: member 1's are null here
    null1 = (C.c_void_p * 2)(lstm[0][0], None)
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(100, 256), null1, *lstm[1:], wpp, bpp, lsp, 0, C.byref(h)) == INVALID
    assert msg().startswith("rdv_param_groups_check:") and "group 0 has size 100" in msg()
    assert lib.rdv_lstm_critic_set_create(C.byref(ok), 2, sizes(256, 0), *lstm, wpp, bpp, 0, C.byref(h)) == INVALID and "group 1 has size 0" in msg()
    # a null member array names the member
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(256, 37), null1, *lstm[1:], wpp, bpp, lsp, 0, C.byref(h)) == INVALID
    assert "rdv_lstm_policy_set_create: member 1" in msg() and "null" in msg()
    nullw = (C.c_void_p * 2)(None, wpp[1])
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(256, 37), *lstm, nullw, bpp, lsp, 0, C.byref(h)) == INVALID and "member 0" in msg()
    nulls = (C.c_void_p * 2)(lsp[0], None)
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(256, 37), *lstm, wpp, bpp, nulls, 0, C.byref(h)) == INVALID and "member 1" in msg() and "log_std" in msg()
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(256, 37), *lstm, wpp, bpp, None, 0, C.byref(h)) == INVALID
    # a non-finite weight names the member: in the LSTM, and in a trunk layer
    with torch.no_grad():
        members[1].lstm_actor.weight_hh_l0[3, 3] = float("inf")
    lstm, wpp, bpp, lsp, keep = _c_arrays(members)
    assert lib.rdv_lstm_policy_set_create(C.byref(ok), 2, sizes(256, 37), *lstm, wpp, bpp, lsp, 0, C.byref(h)) == BAD_PARAMS
    assert "member 1" in msg() and "non-finite LSTM weight" in msg()
    members = [_member(32, 0), _member(32, 1)]
    with torch.no_grad():
        members[0].v2.weight[1, 1] = float("nan")
    lstm, wpp, bpp, _, keep = _c_arrays(members, "v")
    assert lib.rdv_lstm_critic_set_create(C.byref(ok), 2, sizes(256, 37), *lstm, wpp, bpp, 0, C.byref(h)) == BAD_PARAMS
    assert "member 0" in msg() and "non-finite weight in trunk layer 1" in msg()
    # the new calls on no handle
    assert lib.rdv_lstm_set_member_weights(None, 0, None, None, None, None, None, None, None, None) == -5       # RDV_ERR_BAD_HANDLE


# ---------------------------------------------------------------------------------------------------------------- the build
SET_CELL = [f"lstm_cell_kernelILi{H}EJNS_13LstmSetBlocksEEEE" for H in (32, 64, 128, 256)]
SET_TRUNK = [f"lstm_trunk_kernelILi{a}ELb{c}EJNS_13LstmSetBlocksEEEE" for a in (0, 1, 2) for c in (0, 1)]


def test_resource_report_holds_the_set_forms():
    """`make resource` (hipcc's kernel-resource remarks, gfx950 cross-compile, the Makefile's flags) for the recurrent unit: the four
    set cell kernels and the six set trunk kernels beside the eleven plain ones, each without scratch and within 256 VGPRs (two waves
    per SIMD, as the plain cell kernels at 210 to 237)."""
    make = open(os.path.join(N.CSRC, "Makefile")).read()
    assert re.search(r"kernel-resource-usage -c -o /dev/null rdv_policy_lstm\.hip", make)       # the line `make resource` runs for the unit
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_diff as K
    hipcc, flags = K.hipflags(N.CSRC)
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "rdv_policy_lstm.hip"], cwd=N.CSRC,
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
    assert len(vgprs) == 21 and set(vgprs) == set(scratch), sorted(vgprs)
    for w in SET_CELL + SET_TRUNK:
        hits = [k for k in vgprs if w in k]
        assert len(hits) == 1, (w, sorted(vgprs))
        assert scratch[hits[0]] == 0 and vgprs[hits[0]] <= 256, (w, scratch[hits[0]], vgprs[hits[0]])


def test_recurrent_kernels_are_what_the_record_says():
    """profiles/lstm_sets_isa_diff.md records, for the four lstm_cell_kernels, the six lstm_trunk_kernels and lstm_reset_kernel, that the
    parent's and this tree's gfx950 instruction streams are identical, with a digest of each stream, and the streams of the ten set
    forms.  This tree's rdv_policy_lstm.hip, compiled again, still gives those digests."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_diff as K
    rows = re.findall(r"^\| (\w+): `([^`]+)` \| (\d+|-) \| (\d+) \| `(\w+)` \| (\w+) \|$", open(os.path.join(ROOT, "profiles", "lstm_sets_isa_diff.md")).read(), re.M)
    old, new = [r for r in rows if r[5] == "yes"], [r for r in rows if r[5] == "new"]
    assert len(rows) == 21 and len(old) == 11 and len(new) == 10 and all(r[0] == "rdv_policy_lstm" for r in rows), rows
    assert all(r[2] == r[3] and "LstmSetBlocks" not in r[1] for r in old) and all(r[2] == "-" and "rdv::LstmSetBlocks>" in r[1] for r in new)
    assert sorted(r[1].split("::")[1].split("<")[0] for r in old) == ["lstm_cell_kernel"] * 4 + ["lstm_reset_kernel"] + ["lstm_trunk_kernel"] * 6
    got = K.streams("rdv_policy_lstm")
    assert sorted(got) == sorted(r[1] for r in rows)
    for _, name, _, count, sha, _ in rows:
        assert (len(got[name]), K.digest(got[name])) == (int(count), sha), name
    # the same eleven digests stand in the earlier record of the unit
    earlier = open(os.path.join(ROOT, "profiles", "policy_host_isa_diff.md")).read()
    for _, name, _, count, sha, _ in old:
        assert f"`{name}` | {count} | {count} | `{sha}` | yes |" in earlier, name

"""
GPU tests (run with `-m gpu`) of the recurrent policy's kernels (csrc/rdv_policy_lstm.h; rdv_lstm_* in include/rdv.h) against the
float64 NumPy reference of tests/policy_lstm_reference.py: H in {32, 64, 128, 256}, actor and critic, 6 steps with episode starts on
steps 0, 2 and 3, means / values and the state (h, c) after every step within

    e_hip <= 1.5 e32 + A            e32 = max|float32 run - float64 run|, A = the first-order entrywise budget through the cell and the
                                    trunk (policy_lstm_reference.budget), both from the reference alone, over the rows of the case

and, since that budget grows with every step it is carried through (at 64 steps it asserts nothing), the LOCAL check: (h, c) is
downloaded before a step, and the step's output and new state are held to the float64 reference of that ONE step from that downloaded
state, within policy_lstm_reference.local_budget's 1.5 e32 + A — the same at step 60 as at step 0, along the device's own trajectory.
It carries the classes of the scaling corners (s_ih != s_hh), saturated gates and large |c|, a 64-step trajectory and the states that
only rdv_lstm_set_state can put there.  Then the noise, the state calls, rdv_rollout and rdv_rollout_advantages against the loops they
are defined by, the NaN rule and the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import advantages_reference as AR
import policy_lstm_reference as L
import policy_reference as R
from helpers import gpu_batch
from policy_set_cases import DEV, dev as _dev, lstm_loop, short_episodes as _short_episodes, stagger as _stagger, stream as _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_MAX = max(L.BATCH_SIZES)


def _policy(net, critic, n_rows, seed=0):
    from reinforcement_learning_rendezvous_amd import LstmPolicy
    p = LstmPolicy(L.weights_dict(net, critic), activation_fn=net["act"], n_rows=n_rows).to(DEV)
    p.noise_seed = seed
    return p


def _state(pol, kind):
    h, c = pol.state if kind == "actor" else pol.critic_state
    return h.cpu().numpy(), c.cpu().numpy()


def _check_local(tag, kind, net, obs_t, starts_t, before, got, after, t, worst, failures):
    """One step against the float64 reference of that step from the state `before` = (h, c) as downloaded in front of it: the output
    `got` [n, out_dim] (an actor's is clipped, and so is the reference's: the clip is 1-Lipschitz) and the state `after`, each within
    the one-step tolerance over the rows of the call.  `worst` = [ratio, err, tol, where] keeps the largest ratio seen."""
    bud = L.local_budget(net, obs_t, starts_t, before[0], before[1])
    want = np.clip(bud["out64"], -1.0, 1.0) if kind == "actor" else bud["out64"]
    for what, g, w in (("out", got, want), ("h", after[0].astype(np.float64), bud["h64"]), ("c", after[1].astype(np.float64), bud["c64"])):
        err, tol = float(np.abs(g - w).max()), L.local_tolerance(bud, what)
        if not err / tol < worst[0]:
            worst[:] = [err / tol, err, tol, f"{tag}/step {t}/{what}"]
        if not err <= tol:
            failures.append((tag, "local", t, what, err, tol, "row", int(np.abs(g - w).max(axis=1).argmax())))
    return bud


def _check_steps(tag, pol, kind, net, bud, obs, starts, n, worst, failures, local=None):
    """T steps of the actor (deterministic) or critic on the first n rows; every step's output and state against the budget's slice.
    `local`: a `worst` list of its own — the local check of every step (_check_local) on top."""
    T = obs.shape[0]
    tol = {w: L.tolerance(bud, w, n) for w in ("out", "h", "c")}
    for t in range(T):
        o, s = _dev(obs[t, :n]), starts[t, :n]
        before = _state(pol, kind) if local is not None else None
        if kind == "actor":
            got = pol.act(o, episode_start=s, deterministic=True).cpu().numpy().astype(np.float64)
            want = np.clip(bud["out64"][t, :n], -1.0, 1.0)
            h, c = pol.state
        else:
            got = pol.value(o, episode_start=s).cpu().numpy().astype(np.float64)[:, None]
            want = bud["out64"][t, :n]
            h, c = pol.critic_state
        assert got.shape == want.shape and np.isfinite(got).all(), (tag, t)
        for what, g, w in (("out", got, want), ("h", h.cpu().numpy().astype(np.float64), bud["h64"][t, :n]),
                           ("c", c.cpu().numpy().astype(np.float64), bud["c64"][t, :n])):
            err = float(np.abs(g - w).max())
            ratio = err / tol[what][t]
            if ratio >= worst[0]:
                worst[:] = [ratio, err, float(tol[what][t]), f"{tag}/step {t}/{what}"]
            if not err <= tol[what][t]:
                failures.append((tag, t, what, err, float(tol[what][t]), "row", int(np.abs(g - w).max(axis=1).argmax())))
        if local is not None:
            _check_local(tag, kind, net, obs[t, :n], s, before, got, (h.cpu().numpy(), c.cpu().numpy()), t, local, failures)


@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_steps_against_fp64(H):
    """[64, 64] tanh trunk; both network classes; rows on both sides of the 32-env wave tile and the 256-env workgroup; actor and critic.
    At n = 257 every step is also held to the one-step reference from the state in front of it: steps 3 to 5 of `hot`, where the global
    tolerance on the means has passed the clip's width, assert something."""
    obs, starts = L.obs_sequence(N_MAX), L.episode_starts(N_MAX)
    failures = []
    for cid, make in L.CLASSES.items():
        net, critic = make(H), L.critic_of(make(H, seed=77))
        buds = {"actor": L.budget(net, obs, starts), "critic": L.budget(critic, obs, starts)}
        worst = {"actor": [0.0, 0.0, 0.0, ""], "critic": [0.0, 0.0, 0.0, ""]}
        local = {"actor": [0.0, 0.0, 0.0, ""], "critic": [0.0, 0.0, 0.0, ""]}
        for n in L.BATCH_SIZES:
            pol = _policy(net, critic, n)
            for kind, nn in (("actor", net), ("critic", critic)):
                _check_steps(f"{cid}/n{n}/{kind}", pol, kind, nn, buds[kind], obs, starts, n, worst[kind], failures, local[kind] if n == 257 else None)
            pol.close()
        for kind, w in worst.items():
            print(f"TABLE H {H:3d} {cid:12s} {kind:6s} e_hip {w[1]:.3g}  bound {w[2]:.3g}  ({w[3]}: {w[0]:.2f} of its bound)")
            print(f"TABLE H {H:3d} {cid:12s} {kind:6s} local e_hip {local[kind][1]:.3g}  bound {local[kind][2]:.3g}  ({local[kind][3]}: {local[kind][0]:.2f} of its bound)")
    assert not failures, failures[:8]


# ------------------------------------------------------------------------------- scaling corners, long runs, state corners
LOCAL_ROWS = 65                                  # two full 32-row wave tiles and one row of a third


@pytest.mark.parametrize("cid", list(L.NEW_CLASSES))
@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_new_classes_against_fp64(H, cid):
    """The classes whose cell has s_ih != s_hh, gates at 0 and 1 and a large |c|: 6 steps, actor and critic, the budget along the run and
    the one-step reference at every step; then ONE step from the state a float32 run reaches after 48 steps (big_bias: |c| near 48), put
    there by set_state."""
    n = LOCAL_ROWS
    obs, starts = L.obs_sequence(n), L.episode_starts(n)
    make = L.NEW_CLASSES[cid]
    net, critic = make(H), L.critic_of(make(H, seed=77))
    pol = _policy(net, critic, n)
    failures = []
    for kind, nn in (("actor", net), ("critic", critic)):
        worst, local = [0.0, 0.0, 0.0, ""], [0.0, 0.0, 0.0, ""]
        _check_steps(f"{cid}/{kind}", pol, kind, nn, L.budget(nn, obs, starts), obs, starts, n, worst, failures, local)
        far_obs, h0, c0 = L.far_state(nn, n)
        if kind == "actor":
            pol.state = (_dev(h0), _dev(c0))
            got = pol.act(_dev(far_obs), deterministic=True).cpu().numpy().astype(np.float64)
        else:
            pol.critic_state = (_dev(h0), _dev(c0))
            got = pol.value(_dev(far_obs)).cpu().numpy().astype(np.float64)[:, None]
        _check_local(f"{cid}/{kind}", kind, nn, far_obs, None, (h0, c0), got, _state(pol, kind), L.FAR_T, local, failures)
        print(f"TABLE H {H:3d} {cid:12s} {kind:6s} local e_hip {local[1]:.3g}  bound {local[2]:.3g}  ({local[3]}: {local[0]:.2f} of its bound)")
    pol.close()
    assert not failures, failures[:8]


LONG_T = 64


def _long_starts(n, T=LONG_T, seed=63):
    """([T, n] episode starts: Bernoulli(0.1) per row and step, every row at steps 0 and 40; the steps called with episode_start=None)"""
    s = (np.random.default_rng(seed).random((T, n)) < 0.1).astype(np.uint8)
    s[0] = s[40] = 1
    none = [t for t in range(T) if t % 9 == 5]
    s[none] = 0
    return s, none


@pytest.mark.parametrize("cid", ("hot", "long_memory"))
@pytest.mark.parametrize("H", (32, 256))
def test_a_trajectory_of_64_steps(H, cid):
    """64 steps of actor and critic along the device's own trajectory, every step held to the one-step reference from the state in front
    of it (a lost or stale commit of h' or c' is an error of the size of the state); every eighth critic step is preceded by a
    commit=False peek on another observation, which leaves the state — and, against a twin that never peeks, every later value —
    bit-equal.  The error against the free-running float64 run is only required to stay finite: its budget is 1e39 by now."""
    n, T = LOCAL_ROWS, LONG_T
    obs = L.obs_sequence(n, T)
    starts, none = _long_starts(n)
    make = L.ALL_CLASSES[cid]
    net, critic = make(H), L.critic_of(make(H, seed=77))
    pol, twin = _policy(net, critic, n), _policy(net, critic, n)
    free = {"actor": L.run(net, obs, starts)[0], "critic": L.run(critic, obs, starts)[0]}
    failures, peeks = [], 0
    worst = {"actor": [0.0, 0.0, 0.0, ""], "critic": [0.0, 0.0, 0.0, ""]}
    drift = {"actor": 0.0, "critic": 0.0}
    for t in range(T):
        o, s = _dev(obs[t]), (None if t in none else starts[t])
        for kind, nn in (("actor", net), ("critic", critic)):
            before = _state(pol, kind)
            if kind == "critic" and t % 8 == 3:
                other = obs[(t + 7) % T]
                peek = pol.value(_dev(other), episode_start=s, commit=False).cpu().numpy().astype(np.float64)[:, None]
                held = _state(pol, kind)
                assert np.array_equal(before[0], held[0]) and np.array_equal(before[1], held[1]), (t, "the peek wrote the state")
                ref = L.local_budget(nn, other, starts[t], before[0], before[1])
                assert np.abs(peek - ref["out64"]).max() <= L.local_tolerance(ref, "out"), (t, "peek")
                peeks += 1
            if kind == "actor":
                got = pol.act(o, episode_start=s, deterministic=True).cpu().numpy().astype(np.float64)
                assert (np.abs(got) < 1.0).any(), (t, "every mean is clipped")
                want = np.clip(free[kind][t], -1.0, 1.0)
            else:
                v = pol.value(o, episode_start=s)
                assert torch.equal(v, twin.value(o, episode_start=s)), (t, "a peek changed the trajectory")
                got = v.cpu().numpy().astype(np.float64)[:, None]
                want = free[kind][t]
            _check_local(f"{cid}/{kind}", kind, nn, obs[t], starts[t], before, got, _state(pol, kind), t, worst[kind], failures)
            assert np.isfinite(got).all(), (t, kind)
            drift[kind] = max(drift[kind], float(np.abs(got - want).max()))
    for x, y in zip(pol.critic_state, twin.critic_state):
        assert torch.equal(x, y)
    for kind, w in worst.items():
        print(f"TABLE H {H:3d} {cid:12s} {kind:6s} {T} steps  worst local ratio {w[0]:.2f} at {w[3]} (e_hip {w[1]:.3g}, bound {w[2]:.3g})  "
              f"global drift {drift[kind]:.3g}")
    pol.close(); twin.close()
    assert peeks == 8 and len(none) >= 5 and np.isfinite(list(drift.values())).all()
    assert not failures, failures[:8]


def test_state_corners_through_set_state():
    """|h| at and beyond the +-63 clamp, +-inf, -0.0, and |c| up to 1e30 (policy_lstm_reference.state_corners), put there by
    rdv_lstm_set_state: one step of actor and critic, every row held to the one-step reference — which clamps h where it enters W_hh h
    and nowhere else — within that ROW's tolerance (a row with c = 1e30 has a tolerance of its own size); and the rows that keep the
    ordinary state have the bits they have when every row is ordinary."""
    H = 64
    net, critic = L.hot(H), L.critic_of(L.hot(H, seed=77))
    failures = []
    for kind, nn in (("actor", net), ("critic", critic)):
        sc = L.state_corners(nn)
        n = len(sc["obs"])
        o = _dev(sc["obs"])
        step = (lambda p: p.act(o, deterministic=True)) if kind == "actor" else (lambda p: p.value(o)[:, None])
        results = {}
        for name, (h0, c0) in (("corners", (sc["h"], sc["c"])), ("ordinary", (sc["h_ord"], sc["c_ord"]))):
            pol = _policy(net, critic, n)
            state = (_dev(h0), _dev(c0))
            if kind == "actor":
                pol.state = state
            else:
                pol.critic_state = state
            back = _state(pol, kind)
            assert np.array_equal(back[0], h0, equal_nan=True) and np.array_equal(back[1], c0) and np.array_equal(np.signbit(back[0]), np.signbit(h0))
            got = step(pol).cpu().numpy()
            results[name] = (got,) + _state(pol, kind)
            pol.close()
        got, h1, c1 = results["corners"]
        bud = L.local_budget(nn, sc["obs"], None, sc["h"], sc["c"])
        want = np.clip(bud["out64"], -1.0, 1.0) if kind == "actor" else bud["out64"]
        for r in range(n):
            line = [f"TABLE corner {kind:6s} row {r:2d} {sc['kind'][r]:9s}"]
            for what, g, w in (("out", got, want), ("h", h1, bud["h64"]), ("c", c1, bud["c64"])):
                err, tol = float(np.abs(g[r].astype(np.float64) - w[r]).max()), L.local_tolerance(bud, what, [r])
                line.append(f"{what} {err:.3g} / {tol:.3g}")
                if not err <= tol:
                    failures.append((kind, r, sc["kind"][r], what, err, tol))
            print("  ".join(line))
        for a, b in zip(results["corners"], results["ordinary"]):
            assert np.array_equal(a[sc["ordinary"]], b[sc["ordinary"]]), (kind, "an ordinary row beside a corner row changed")
    assert not failures, failures


@pytest.mark.parametrize("arch,act", L.EXTRA_TRUNKS, ids=[f"{'x'.join(map(str, a))}-{f}" for a, f in L.EXTRA_TRUNKS])
@pytest.mark.parametrize("H", (64, 256))
def test_other_trunks_against_fp64(H, arch, act):
    n = 257
    obs, starts = L.obs_sequence(n), L.episode_starts(n)
    net, critic = L.hot(H, arch, act), L.critic_of(L.default_init(H, arch, act, seed=78))
    pol = _policy(net, critic, n)
    failures = []
    for kind, nn in (("actor", net), ("critic", critic)):
        worst = [0.0, 0.0, 0.0, ""]
        _check_steps(f"{kind}", pol, kind, nn, L.budget(nn, obs, starts), obs, starts, n, worst, failures)
        print(f"TABLE H {H:3d} {'x'.join(map(str, arch)):12s} {act:8s} {kind:6s} e_hip {worst[1]:.3g}  bound {worst[2]:.3g}  ({worst[3]}: {worst[0]:.2f} of its bound)")
    pol.close()
    assert not failures, failures[:8]


@pytest.mark.parametrize("H", L.HIDDEN_SIZES)
def test_routing_probes(H):
    """One non-zero weight per gate row in W_ih and in W_hh: over the probes every (gate, tile, k-step) fragment carries one."""
    n = 65
    obs, starts = L.obs_sequence(n, 3), L.episode_starts(n, 3)
    failures = []
    for m in range(L.ROUTE_PROBES):
        net = L.route_probe(H, m)
        pol = _policy(net, L.critic_of(net), n)
        worst = [0.0, 0.0, 0.0, ""]
        _check_steps(f"probe {m}", pol, "actor", net, L.budget(net, obs, starts), obs, starts, n, worst, failures)
        pol.close()
    assert not failures, failures[:8]


# ------------------------------------------------------------------------------------------------------------- the noise
def _noise_net(H=64):
    net = L.default_init(H)
    return dict(net, log_std=np.asarray((-5.0, -0.5, 0.0, 1.0, -0.5, 0.0), np.float32))


def test_stochastic_act_against_philox_reference():
    """Unclipped sample, clipped action and log_prob of one stochastic step against mean64 + exp(log_std) z_ref and log_prob64, with the
    tolerances of test_gpu_policy_mlp.py; two handles over rows [0, 512) and [512, 1000) with env_id_offset equal one handle of 1000."""
    n, seed, ctr, off = 1000, 0xABCDEF12345, 7, 2 ** 33 + 5
    net = _noise_net()
    obs, starts = L.obs_sequence(n, 1), L.episode_starts(n, 1)
    bud = L.budget(net, obs, starts)
    pol = _policy(net, L.critic_of(net), n, seed=seed)
    pol._calls = ctr
    raw = torch.empty((n, 6), dtype=torch.float32, device=DEV)
    lp = torch.empty((n,), dtype=torch.float32, device=DEV)
    clipped = pol.act(_dev(obs[0]), episode_start=starts[0], deterministic=False, env_id_offset=off, raw_out=raw, log_prob_out=lp)
    ids = (off + np.arange(n)).astype(np.uint64)
    z = R.actor_normals(seed, ids, ctr)
    std = np.exp(net["log_std"].astype(np.float64))
    want = bud["out64"][0] + std * z
    tol = L.tolerance(bud, "out")[0] + std * R.TOL_Z
    err = np.abs(raw.cpu().numpy().astype(np.float64) - want)
    assert (err <= tol).all(), ("unclipped sample", float((err / tol).max()))
    far = (np.abs(want - 1.0) > tol) & (np.abs(want + 1.0) > tol)
    cl = clipped.cpu().numpy()
    errc = np.abs(cl.astype(np.float64) - np.clip(want, -1.0, 1.0))
    assert far.mean() > 0.9 and (errc[far] <= np.broadcast_to(tol, errc.shape)[far]).all() and (np.abs(cl) <= 1.0).all()
    lp64 = R.log_prob64(z, net["log_std"])
    tol_lp = 6.0 * np.abs(z).max(axis=1) * R.TOL_Z + 4e-6 * (1.0 + np.abs(lp64))
    assert (np.abs(lp.cpu().numpy().astype(np.float64) - lp64) <= tol_lp).all()
    # the same rows through two handles
    parts = []
    for lo, hi in ((0, 512), (512, 1000)):
        part = _policy(net, L.critic_of(net), hi - lo, seed=seed)
        part._calls = ctr
        r = torch.empty((hi - lo, 6), dtype=torch.float32, device=DEV)
        q = torch.empty((hi - lo,), dtype=torch.float32, device=DEV)
        a = part.act(_dev(obs[0, lo:hi]), episode_start=starts[0, lo:hi], deterministic=False, env_id_offset=off + lo, raw_out=r, log_prob_out=q)
        parts.append((a, r, q, part.state))
        part.close()
    assert torch.equal(torch.cat([p[0] for p in parts]), clipped) and torch.equal(torch.cat([p[1] for p in parts]), raw)
    assert torch.equal(torch.cat([p[2] for p in parts]), lp)
    for i in range(2):
        assert torch.equal(torch.cat([p[3][i] for p in parts]), pol.state[i])
    pol.close()


# ---------------------------------------------------------------------------------------------------------- the state calls
def test_state_calls():
    """commit = 0 leaves (h, c) bit-equal; set_state(get_state()) is the identity; reset_state(mask) touches only masked rows."""
    H, n = 128, 300
    net, critic = L.hot(H), L.critic_of(L.hot(H, seed=5))
    pol = _policy(net, critic, n)
    obs, starts = L.obs_sequence(n, 3), L.episode_starts(n, 3)
    for t in range(2):
        pol.act(_dev(obs[t]), episode_start=starts[t]); pol.value(_dev(obs[t]), episode_start=starts[t])
    h, c = pol.critic_state
    peek = pol.value(_dev(obs[2]), episode_start=starts[2], commit=False)
    h1, c1 = pol.critic_state
    assert torch.equal(h, h1) and torch.equal(c, c1)
    assert torch.equal(pol.value(_dev(obs[2]), episode_start=starts[2]), peek)          # ... and is what the committing call computes
    assert not torch.equal(pol.critic_state[0], h)
    ah, ac = pol.state
    assert float(ah.abs().max()) > 0.01
    pol.state = (ah, ac)
    assert torch.equal(pol.state[0], ah) and torch.equal(pol.state[1], ac)
    a1 = pol.act(_dev(obs[2]))
    pol.state = (ah, ac)
    assert torch.equal(pol.act(_dev(obs[2])), a1)                                         # the state IS what the step reads
    ah, ac = pol.state
    mask = torch.from_numpy((np.arange(n) % 7 == 3).astype(np.uint8)).to(DEV)
    pol.reset_state(mask)
    h2, c2 = pol.state
    m = mask.bool()
    assert (h2[m] == 0).all() and (c2[m] == 0).all() and torch.equal(h2[~m], ah[~m]) and torch.equal(c2[~m], ac[~m])
    assert (pol.critic_state[0][m] == 0).all()
    pol.reset_state()
    assert float(pol.state[0].abs().max()) == 0.0 and float(pol.critic_state[1].abs().max()) == 0.0
    pol.close()


def test_update_weights_equals_a_fresh_policy_and_keeps_the_state():
    H, n = 64, 100
    net, critic, net2, critic2 = L.default_init(H), L.critic_of(L.default_init(H, seed=3)), L.hot(H, seed=4), L.critic_of(L.hot(H, seed=6))
    obs, starts = L.obs_sequence(n, 2), L.episode_starts(n, 2)
    pol, fresh = _policy(net, critic, n), _policy(net2, critic2, n)
    pol.act(_dev(obs[0]), episode_start=starts[0]); pol.value(_dev(obs[0]), episode_start=starts[0])
    fresh.state = pol.state; fresh.critic_state = pol.critic_state
    pol.update_weights(L.weights_dict(net2, critic2))
    assert torch.equal(pol.act(_dev(obs[1])), fresh.act(_dev(obs[1]))) and torch.equal(pol.value(_dev(obs[1])), fresh.value(_dev(obs[1])))
    assert torch.equal(pol.state[0], fresh.state[0])
    from reinforcement_learning_rendezvous_amd import _native as N
    bad = L.weights_dict(net2, critic2); bad["lstm_actor.weight_hh_l0"] = bad["lstm_actor.weight_hh_l0"].copy(); bad["lstm_actor.weight_hh_l0"][3, 3] = np.inf
    with pytest.raises(N.RdvError, match="non-finite"):
        pol.update_weights(bad)
    pol.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------ rollout and collect
def test_rollout_is_the_lstm_act_plus_step_loop_and_continues():
    """300 envs x 12 steps, episodes of 4 steps: rdv_rollout with an LSTM actor against the explicit loop — every column, last_obs, the
    final state and the pending flags by equality; two rollouts of 6 steps equal one of 12."""
    n, T, seed, ctr0, off, H = 300, 12, 41, 9, 700, 64
    net = _noise_net(H)
    critic = L.critic_of(L.hot(H, seed=8))
    envs = [gpu_batch(n, params=_short_episodes(), seed=13, env_id_offset=off) for _ in range(3)]
    pols = [_policy(net, critic, n, seed=seed) for _ in range(3)]
    for e in envs:
        e.reset()
        _stagger(e)
    pols[0]._calls = ctr0
    ro = envs[0].rollout(pols[0], T)
    assert envs[0].last_kernel.startswith("step_kernel") and pols[0]._calls == ctr0 + T
    assert int(ro["done"].sum()) >= 2 * n and int(ro["done"][:-1].sum()) > 0            # episodes end inside the rollout
    loop, last_flags = lstm_loop(envs[1], pols[1], T, ctr0)
    for k in ("obs", "actions", "reward", "done", "log_prob", "last_obs"):
        assert torch.equal(ro[k].to(loop[k].dtype), loop[k]), k
    assert float(ro["lstm_state0"][0].abs().max()) == 0.0                                # every row was pending: step 0 starts from zero
    pols[2]._calls = ctr0
    first = envs[2].rollout(pols[2], T // 2)
    first = {k: (tuple(x.clone() for x in v) if isinstance(v, tuple) else v.clone()) for k, v in first.items()}
    mid_state = pols[2].state_at_start("l", DEV)
    second = envs[2].rollout(pols[2], T // 2)
    for k in ("obs", "actions", "reward", "done", "log_prob"):
        assert torch.equal(torch.cat([first[k], second[k]]), ro[k]), k
    assert torch.equal(second["last_obs"], ro["last_obs"])
    for x, y in zip(second["lstm_state0"], mid_state):
        assert torch.equal(x, y)
    keep = (first["done"][-1] == 0)
    assert 0 < int(keep.sum()) < n                                                       # some envs, not all, finished at the last step of the first half
    assert float(second["lstm_state0"][0][~keep].abs().max()) == 0.0 and float(second["lstm_state0"][0][keep].abs().max()) > 0.0
    for p in pols[1:]:
        for x, y in zip(p.state, pols[0].state):
            assert torch.equal(x, y)
    # the pending flags on the handle are done[T-1]: a deterministic step with no flags of its own differs from one that uses them
    for e, p in zip(envs, pols):
        assert torch.equal(e.get_state(), envs[0].get_state())
    nxt = envs[0].rollout(pols[0], 1, deterministic=True)
    pols[1]._calls = ctr0 + T
    want = pols[1].act(loop["last_obs"], episode_start=last_flags, deterministic=True, env_id_offset=off)
    assert torch.equal(nxt["actions"][0].clamp(-1.0, 1.0), want)
    for e in envs:
        e.close()
    for p in pols:
        p.close()


def test_collect_is_the_critic_loop_plus_gae():
    n, T, H = 300, 12, 32
    net, critic = _noise_net(H), L.critic_of(L.hot(H, seed=8))
    env = gpu_batch(n, params=_short_episodes(), seed=13)
    env.reset()
    pol, twin = _policy(net, critic, n, seed=5), _policy(net, critic, n, seed=5)
    last_done = None
    for call in range(2):
        ro = env.collect(pol, T // 2, gamma=0.97, gae_lambda=0.92)
        flags = np.ones(n, np.uint8) if call == 0 else last_done
        values = []
        for t in range(T // 2):
            values.append(twin.value(ro["obs"][t].contiguous(), episode_start=flags).clone())
            flags = ro["done"][t].cpu().numpy()
        last_value = twin.value(ro["last_obs"], episode_start=flags, commit=False)
        last_done = flags
        values = torch.stack(values)
        assert torch.equal(ro["values"], values) and torch.equal(ro["last_value"], last_value)
        adv, ret = AR.gae32(ro["reward"].cpu().numpy(), ro["done"].cpu().numpy(), values.cpu().numpy(), last_value.cpu().numpy(), 0.97, 0.92)
        np.testing.assert_array_equal(ro["advantages"].cpu().numpy(), adv)
        np.testing.assert_array_equal(ro["returns"].cpu().numpy(), ret)
        for x, y in zip(pol.critic_state, twin.critic_state):
            assert torch.equal(x, y)
    env.close(); pol.close(); twin.close()


def test_collect_with_rows_that_are_no_multiple_of_four():
    """n = 33: row t of [T, N, 17] is not 16-byte aligned; the critic reads it through its aligned scratch rows."""
    n, T, H = 33, 3, 32
    net, critic = _noise_net(H), L.critic_of(L.hot(H, seed=8))
    env = gpu_batch(n, params=_short_episodes(), seed=3)
    env.reset()
    pol, twin = _policy(net, critic, n), _policy(net, critic, n)
    ro = env.collect(pol, T)
    flags = np.ones(n, np.uint8)
    for t in range(T):
        assert torch.equal(ro["values"][t], twin.value(ro["obs"][t].contiguous(), episode_start=flags))
        flags = ro["done"][t].cpu().numpy()
    env.close(); pol.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- NaN rule and refusals
def test_a_nan_row_poisons_only_its_own_row_and_state():
    H, n = 256, 256
    net, critic = L.hot(H), L.critic_of(L.hot(H, seed=2))
    obs, starts = L.obs_sequence(n, 2), L.episode_starts(n, 2)
    clean = _policy(net, critic, n)
    a0 = [clean.act(_dev(obs[t]), episode_start=starts[t]).clone() for t in range(2)]
    v0 = [clean.value(_dev(obs[t]), episode_start=starts[t]).clone() for t in range(2)]
    h0, c0 = clean.state
    assert all(torch.isfinite(x).all() for x in a0 + v0)
    for r, k in ((0, 0), (31, 16), (32, 7), (255, 12)):
        pol = _policy(net, critic, n)
        bad = obs[0].copy(); bad[r, k] = np.nan
        a = [pol.act(_dev(bad), episode_start=starts[0]), pol.act(_dev(obs[1]), episode_start=starts[1])]     # step 1: through the state
        v = [pol.value(_dev(bad), episode_start=starts[0]), pol.value(_dev(obs[1]), episode_start=starts[1])]
        keep = torch.arange(n, device=DEV) != r
        for t in range(2):
            assert torch.isnan(a[t][r]).all() and torch.isnan(v[t][r]), (r, k, t)
            assert torch.equal(a[t][keep], a0[t][keep]) and torch.equal(v[t][keep], v0[t][keep]), (r, k, t)
        h, c = pol.state
        assert torch.isnan(h[r]).all() and torch.equal(h[keep], h0[keep]) and torch.equal(c[keep], c0[keep])
        pol.close()
    clean.close()


def test_refusals():
    from reinforcement_learning_rendezvous_amd import _native as N
    from reinforcement_learning_rendezvous_amd import LstmPolicy
    lib, n = N.lib(), 64
    net = L.default_init(32)
    pol = _policy(net, L.critic_of(net), n)
    obs = _dev(L.obs_sequence(n, 1)[0])
    pol.act(obs); pol.value(obs)
    actor, critic = pol._hip[0], pol._hip_critic[0]
    assert lib.rdv_lstm_hidden_size(actor) == 32 and lib.rdv_policy_num_rows(critic) == n
    spec = N.MlpSpec()
    N.check(lib.rdv_policy_get_spec(actor, C.byref(spec)))
    assert spec.to_tuple() == (2, [64, 64, 0, 0], N.ACT_TANH)                             # the trunk
    out = torch.empty((n, 6), dtype=torch.float32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    INVALID = -1
    assert lib.rdv_policy_act(actor, p(obs), p(out), n, 1, 0, 0, 0, _stream()) == INVALID and b"recurrent" in lib.rdv_last_error()
    assert lib.rdv_policy_value(critic, p(obs), p(out), n, _stream()) == INVALID and b"recurrent" in lib.rdv_last_error()
    assert lib.rdv_policy_set_weights(actor, None, None, None, _stream()) == INVALID and b"rdv_lstm_set_weights" in lib.rdv_last_error()
    assert lib.rdv_policy_set_member_weights(actor, 0, None, None, None, _stream()) == INVALID
    assert lib.rdv_lstm_act(critic, p(obs), None, p(out), None, None, n, 1, 0, 0, 0, _stream()) == INVALID and b"critic" in lib.rdv_last_error()
    assert lib.rdv_lstm_value(actor, p(obs), None, p(out), n, 1, _stream()) == INVALID and b"actor" in lib.rdv_last_error()
    assert lib.rdv_lstm_act(actor, p(obs), None, p(out), None, None, n - 1, 1, 0, 0, 0, _stream()) == INVALID and b"64 rows" in lib.rdv_last_error()
    from helpers import shipped_policy
    mlp = shipped_policy(device=DEV)
    mlp.act(obs)
    assert lib.rdv_lstm_act(mlp._hip[0], p(obs), None, p(out), None, None, n, 1, 0, 0, 0, _stream()) == INVALID and b"not a recurrent" in lib.rdv_last_error()
    env = gpu_batch(n + 1, seed=1)
    env.reset()
    with pytest.raises(ValueError, match="rows"):
        env.rollout(pol, 2)
    ro = N.RolloutOut(*[p(torch.empty(4096, device=DEV)) for _ in range(6)])
    assert lib.rdv_rollout(env._h, actor, 2, C.byref(ro), 1, 0, 0, _stream()) == INVALID and b"owns 64 rows" in lib.rdv_last_error()
    for kw, word in ((dict(lstm_hidden_size=48), "lstm_hidden_size = 48"), (dict(n_lstm_layers=2), "n_lstm_layers"), (dict(shared_lstm=True), "shared_lstm"),
                     (dict(enable_critic_lstm=False), "enable_critic_lstm")):
        with pytest.raises(ValueError, match=word):
            LstmPolicy(**kw)
    env.close(); mlp.close(); pol.close()

"""
GPU tests (run with `-m gpu`) of the shipped step kernels where their lazy branches decide the outcome.

The training-path kernels (step_kernel_split, step_kernel_parts, step_kernel<ST, false>; include/rdv.h) derive the corridor angle
only inside the keep-out-zone sphere and the velocity / rotation errors only near the docking point (csrc/rdv_device.h,
derive_target<kLazy = true>); everything else stays +inf.  Collision flag, success count and bonus reward are computed from those
values, so they are compared here with the CPU oracle on runs that enter the KOZ, dock and earn bonuses — not kernel against kernel,
and never through the evaluator build (diag outputs), which derives everything.  Every step asserts the kernel that ran
(rdv_debug_last_kernel) against the dispatch rules of tests/helpers.py; the comparison with the oracle is tests/parity.py's, with its
full check set on every step.
"""
import numpy as np
import pytest

import parity
from helpers import counter_actions, expect_kernel, gpu_batch, load_golden, oracle_batch, shipped_policy, to_numpy
from reinforcement_learning_rendezvous_amd.params import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class Branches:
    """Counts, from the ORACLE's outputs, the steps on which the lazy branches decided something: an env inside the KOZ outside the
    corridor (collision), a success step, a step that earned the bonus reward (:340-351: inside the sphere, not collided, position
    error below max_rd_error)."""

    def __init__(self, p):
        self.p, self.collisions, self.successes, self.bonus = p, 0, 0, 0

    def add(self, orc, ref, rows):
        """rows: parity.live_rows (reset rows hold the next episode)."""
        dg, aux, s = orc.diagnose()[rows], orc.get_aux()[rows], orc.get_state()[rows]
        self.collisions += int(dg[:, 4].sum())
        self.successes += int(dg[:, 5].sum())
        inside = np.linalg.norm(s[:, 0:3], axis=1) < self.p.koz_radius
        self.bonus += int((inside & (aux[:, 2] == 0) & (dg[:, 0] < self.p.max_rd_error)).sum())

    def check(self, what):
        print(f"{what}: collision steps {self.collisions}, success steps {self.successes}, bonus steps {self.bonus}")
        assert self.collisions > 0 and self.successes > 0 and self.bonus > 0, (what, self.collisions, self.successes, self.bonus)


# the parameters of test_gpu_random_params.py::test_states_inside_the_keep_out_zone_and_parameter_updates and of
# test_gpu_slots.py CASES[5]: episodes start around the docking point, many inside the sphere, some collided / successful at reset
KOZ_PARAMS = {
    "koz-near-port": dict(rc0=np.array([0.0, -2.2, 0.0]), rc0_range=1.5, qt0_range=float(np.radians(60)), t_max=30),
    "koz-radius4": dict(rc0=np.array([0.0, -2.6, 0.0]), rc0_range=1.5, koz_radius=4.0),
}


def _koz_run(p, n, storage, on_done, variant, steps, seed, n_threads=1):
    env = gpu_batch(n, params=p, storage=storage, on_done=on_done, seed=seed, variant=variant)
    orc = oracle_batch(n, p, storage, on_done, seed=seed, n_threads=n_threads)
    parity.check_reset_obs(env.reset(), orc.reset())
    np.testing.assert_array_equal(to_numpy(env.get_aux())[:, [2, 3]], orc.get_aux()[:, [2, 3]])
    br = Branches(p)
    actions = ((counter_actions(seed + 40, t, n) * 0.3).astype(np.float32) for t in range(steps))
    parity.run_against_oracle(env, orc, actions, storage, variant, on_step=lambda orc, ref, t: br.add(orc, ref, parity.live_rows(env, ref)))
    env.close()
    return br


@pytest.mark.parametrize("on_done", ["reset", "halt", "continue"])
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("pname", list(KOZ_PARAMS))
def test_keep_out_zone_parameters_vs_oracle(pname, storage, on_done):
    """Collisions, success steps and bonus rewards on the shipped kernels (split, parts, in-lane) against the oracle."""
    p = make_params(**KOZ_PARAMS[pname])
    for variant in ("split", "fused", "fused_inlane"):
        _koz_run(p, 512, storage, on_done, variant, 24, 21).check(f"{pname} {storage} {on_done} {variant}")


def test_keep_out_zone_above_the_auto_split_limit_runs_parts():
    """65,536 + 77 envs under AUTO: the size threshold itself is pinned (step_kernel_parts), on a KOZ-heavy run."""
    p = make_params(**KOZ_PARAMS["koz-near-port"])
    _koz_run(p, 65536 + 77, "f32", "reset", "auto", 10, 5, n_threads=8).check("koz-near-port f32 reset auto 65613")


@pytest.mark.parametrize("variant", ["split", "fused"])
def test_closed_loop_policy_into_the_keep_out_zone(variant):
    """The shipped MLP policy, deterministic, on the 1000 Monte Carlo initial conditions (monte_carlo.py's setting: dt = 1,
    t_max = 60, halt at done), stepped through the shipped kernel without diag for the whole episode; the same actions replayed into
    the oracle.  Flags, success counts and reasons must be the oracle's, every step."""
    from reinforcement_learning_rendezvous_amd import monte_carlo as mc
    ics = load_golden("mc_initial_conditions.npz")["states"]
    p = mc.make_eval_params()
    s = ics.copy()
    s[:, 6:10] /= np.linalg.norm(s[:, 6:10], axis=1, keepdims=True)
    s[:, 13:17] /= np.linalg.norm(s[:, 13:17], axis=1, keepdims=True)
    n = len(s)
    env = gpu_batch(n, params=p, storage="f32", on_done="halt", variant=variant)
    orc = oracle_batch(n, p, "f32", "halt")
    pol = shipped_policy("cuda:0")
    env.reset(); orc.reset()
    env.set_state(torch.from_numpy(s)); orc.set_state(s)
    obs = env.observe()
    np.testing.assert_array_equal(to_numpy(obs), orc.observe())
    br = Branches(p)
    for t in range(int(round(p.t_max / p.dt))):
        a = pol.act(obs, deterministic=True).contiguous()
        a_np = to_numpy(a).copy()
        obs, r, d = env.step(a)
        expect_kernel(env, variant, after_set_state=t == 0, what=f"step {t}")
        ref = orc.step(a_np)
        parity.check_outputs(env, ref, obs, r, d, t)
        parity.check_diag(env, orc, parity.live_rows(env, ref), t, False)
        parity.check_state(env, orc, "f32", t)
        br.add(orc, ref, parity.live_rows(env, ref))
    assert bool(to_numpy(d).all())
    parity.check_stats(env, orc)
    st = orc.get_stats()
    print(f"closed loop {variant}: {st['successes']} successful / {st['collisions']} collided episodes of {n}")
    br.check(f"closed loop {variant}")


def _vbar_states(p):
    """States that are bit-exact fixed points of a zero-action step: chaser at rest on the V-bar (rc = (0, y, 0), vc = wc = 0),
    target at rest (wt = 0), chaser attitude the identity (capture axis on the target: attitude error 0).  Each kind puts one
    limit on or 1-2 ulp either side of the value; returns (kind, value, state) rows."""
    base = np.zeros(20)
    base[6] = 1.0; base[13] = 1.0

    def around(x, k=2):
        out = [x]
        lo = hi = x
        for _ in range(k):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
        return sorted(out)
    rows = []
    g = load_golden("boundary_diag.npz")                 # its "pos" kind: rc = [0, -2 - x, 0] for x = max_rd_error and 1-2 ulp around
    for k, x, s in zip(g["kind"], g["value"], g["state"]):
        if str(k) == "pos":
            rows.append(("pos", float(x), s.copy()))
    ry = float(p.rd[1])
    for y in around(ry + p.max_rd_error) + around(ry - p.max_rd_error):   # position error |y - rd_y| exactly on the limit, +-1, 2 ulp of y
        s = base.copy(); s[1] = y
        rows.append(("pos-vbar", abs(y - ry), s))
    q90 = [np.cos(np.pi / 4), 0.0, 0.0, np.sin(np.pi / 4)]   # target turned 90 deg about z: the corridor axis leaves the V-bar
    for r in around(p.koz_radius):                         # |rc| on the KOZ radius: collision iff strictly inside (:397)
        s = base.copy(); s[1] = -r; s[13:17] = q90
        rows.append(("koz-vbar", r, s))
    for dth in (-2e-4, -1e-4, -5e-5, 5e-5, 1e-4, 2e-4):    # corridor edge across the V-bar at 3 m: outside the corridor iff dth > 0
        th = p.corridor_half_angle + dth
        s = base.copy(); s[1] = -3.0; s[13:17] = [np.cos(th / 2), 0.0, 0.0, np.sin(th / 2)]
        rows.append(("corridor", dth, s))
    return rows


@pytest.mark.parametrize("variant", ["split", "fused"])
def test_limit_straddling_states_through_the_step_kernels(variant):
    """Fixed-point states on the limits, stepped in continue mode with zero actions and fp64 storage.  Step 1 after set_state runs
    the kRaw kernel; steps 2-6 run the shipped one, and there the state must stay bit-unchanged (which proves the fixed point), and
    collided, the success count, done_reason and the reward must be the oracle's.

    Kinds placed: docking-position error (boundary_diag.npz "pos", and on the V-bar inside and outside the port: the subtraction
    y - rd_y is exact there, so the error IS the placed value), KOZ radius (on the V-bar, target turned away).  Not placeable as a
    fixed point: velocity and rotation-rate errors (boundary_diag "vel", "rot", "*3": a moving or spinning chaser) and the R-bar KOZ
    kind ("koz": off the V-bar, the CW dynamics move it).  The corridor angle is placed a few 1e-5 cosine steps either side of the
    edge, not at the ulp: the reference rounds the cosine to 5 decimals (general.py:179), so an ulp of the angle does not cross it."""
    p = make_params()
    rows = _vbar_states(p)
    kinds = [k for k, _, _ in rows]
    S = np.stack([s for _, _, s in rows])
    n = len(S)
    env = gpu_batch(n, params=p, storage="f64", on_done="continue", variant=variant)
    orc = oracle_batch(n, p, "f64", "continue")
    env.reset(); orc.reset()
    env.set_state(torch.from_numpy(S)); orc.set_state(S)
    zero = np.zeros((n, 6), np.float32)
    first = None
    for t in range(6):
        o, r, d = env.step(torch.from_numpy(zero).cuda())
        expect_kernel(env, variant, after_set_state=t == 0, what=f"step {t}")
        ref = orc.step(zero)
        state = to_numpy(env.get_state())
        if first is None:
            first = state
        else:
            bad = np.flatnonzero(~(state == first).all(axis=1))
            assert bad.size == 0, f"step {t}: not a fixed point: {[kinds[i] for i in bad]}"
        np.testing.assert_allclose(state, orc.get_state(), rtol=0, atol=1e-10, err_msg=f"state, step {t}")
        aux, aux_ref = to_numpy(env.get_aux()), orc.get_aux()
        for col, what in ((2, "collided"), (3, "success count")):
            bad = np.flatnonzero(aux[:, col] != aux_ref[:, col])
            assert bad.size == 0, (what, t, [(kinds[i], rows[i][1], aux[i, col], aux_ref[i, col]) for i in bad])
        np.testing.assert_array_equal(to_numpy(d), ref["done"], err_msg=f"done, step {t}")
        np.testing.assert_array_equal(to_numpy(env.done_reason), ref["done_reason"], err_msg=f"reason, step {t}")
        bad = np.flatnonzero(np.abs(to_numpy(r) - ref["reward"]) > parity.REWARD_TOL * np.maximum(1.0, np.abs(ref["reward"])))
        assert bad.size == 0, ("reward", t, [(kinds[i], rows[i][1], float(to_numpy(r)[i]), float(ref["reward"][i])) for i in bad])
    # both sides of every limit occur in the oracle's outcome (boundary_diag's "pos" rows all round to y = -2.5: on the limit)
    aux_ref, dg_ref = orc.get_aux(), orc.diagnose()
    kinds = np.array(kinds)
    assert (aux_ref[kinds == "pos", 3] > 0).all()
    for kind, col in (("pos-vbar", 3), ("koz-vbar", 2), ("corridor", 2)):
        vals = aux_ref[kinds == kind, col] > 0
        assert vals.any() and not vals.all(), (kind, vals)
    bonus = (ref["reward"] > 2.0)                            # the bonus terms: the attitude term alone is dt * att_coef = 1 here
    print(f"limit states {variant}: collided {int((aux_ref[:, 2] > 0).sum())}, successful {int((aux_ref[:, 3] > 0).sum())}, "
          f"bonus rows {int(bonus.sum())} of {n}")
    assert bonus.any() and dg_ref[:, 4].any() and dg_ref[:, 5].any()
    env.close()


def test_restored_halted_envs_step_on_in_reset_and_continue_modes():
    """A snapshot of a HALT handle with halted envs, restored into RESET and CONTINUE handles: every kernel steps the restored-halted
    envs on (include/rdv.h, rdv_restore), so every path agrees bit for bit — rdv_step in every variant, with and without diag,
    rdv_step_many, and rdv_rollout against act + step."""
    n, K = 1000, 8
    src = gpu_batch(n, storage="f32", on_done="halt", seed=13)
    src.reset()
    for t in range(18):                                 # about half the envs have finished (and halted) by then
        src.step(torch.from_numpy(counter_actions(8, t, n)).cuda())
    halted = to_numpy(src.done).astype(bool)
    assert 50 < halted.sum() < n
    snap = src.snapshot()
    acts = torch.from_numpy(np.stack([counter_actions(9, t, n) for t in range(K)])).cuda()
    for on_done in ("reset", "continue"):
        results = {}
        for path in ("fused", "split", "fused_inlane", "fused_tiles", "diag", "step_many"):
            env = gpu_batch(n, storage="f32", on_done=on_done, seed=13, variant="auto" if path in ("diag", "step_many") else path)
            env.restore(snap)
            before = to_numpy(env.get_state())
            t_before = to_numpy(env.get_aux())[:, 0]
            if path == "step_many":
                out = env.step_many(acts)
                assert env.last_kernel == "step_many_kernel<float, false>", env.last_kernel
                rows = [(out["obs"][k], out["reward"][k], out["done"][k], out["done_reason"][k]) for k in range(K)]
            else:
                rows = []
                for k in range(K):
                    o, r, d = env.step(acts[k], diag=path == "diag")
                    rows.append((o.clone(), r.clone(), d.clone(), env.done_reason.clone()))
            rows = [[to_numpy(x) for x in row] for row in rows]
            after, aux = to_numpy(env.get_state()), to_numpy(env.get_aux())
            # the restored-halted envs took transitions
            assert (after[halted] != before[halted]).any(axis=1).all(), (on_done, path)
            if on_done == "continue":
                np.testing.assert_array_equal(aux[halted, 0], t_before[halted] + K * src.params.dt, err_msg=f"{path}: t")
            results[path] = (rows, after, aux, env.get_stats())
            env.close()
        ref_rows, ref_state, ref_aux, ref_stats = results["fused"]
        for path, (rows, state, aux, stats) in results.items():
            for k in range(K):
                for j, what in enumerate(("obs", "reward", "done", "done_reason")):
                    np.testing.assert_array_equal(rows[k][j], ref_rows[k][j], err_msg=f"{on_done} {path}: {what}, step {k}")
            np.testing.assert_array_equal(state, ref_state, err_msg=f"{on_done} {path}: state")
            np.testing.assert_array_equal(aux, ref_aux, err_msg=f"{on_done} {path}: aux")
            assert stats == ref_stats, (on_done, path)
        # rdv_rollout (its own actions) against act + step on the same restored snapshot
        pol_a, pol_b = shipped_policy("cuda:0"), shipped_policy("cuda:0")
        roll = gpu_batch(n, storage="f32", on_done=on_done, seed=13)
        loop = gpu_batch(n, storage="f32", on_done=on_done, seed=13, variant="split")
        roll.restore(snap); loop.restore(snap)
        out = roll.rollout(pol_a, K)
        assert roll.last_kernel == "rollout_kernel<float, false>", roll.last_kernel
        for k in range(K):
            a = loop.act(pol_b)                            # clipped, as SB3 passes it to the env; the rollout stores the sample
            np.testing.assert_array_equal(to_numpy(a), np.clip(to_numpy(out["actions"][k]), -1, 1), err_msg=f"{on_done} rollout: actions, step {k}")
            o, r, d = loop.step(a)
            np.testing.assert_array_equal(to_numpy(r), to_numpy(out["reward"][k]), err_msg=f"{on_done} rollout: reward, step {k}")
            np.testing.assert_array_equal(to_numpy(d), to_numpy(out["done"][k]), err_msg=f"{on_done} rollout: done, step {k}")
        np.testing.assert_array_equal(to_numpy(roll.get_state()), to_numpy(loop.get_state()), err_msg=f"{on_done} rollout: state")
        assert (to_numpy(roll.get_state())[halted] != to_numpy(src.get_state())[halted]).any(axis=1).all()
        roll.close(); loop.close()
    src.close()

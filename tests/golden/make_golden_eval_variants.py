#!/usr/bin/env python3
"""
Golden fixture for the evaluators under other configurations than the one of make_golden_eval.py (eval_reference_variants.npz): the
reference's own `CustomWandbCallback.evaluate_policy` (custom/custom_callbacks.py:186-300) and `monte_carlo.evaluate`
(monte_carlo.py:94-207), run UNMODIFIED with the shipped MLP policy (NumPy float32 forward) on the unmodified env, under the axes
sensitivity_analysis.py varies (dt, t_max, koz_radius, corridor_half_angle, rc0, wt0, h); inert stand-ins for the absent imports as in
make_golden.py / make_golden_eval.py.

    python tests/golden/make_golden_eval_variants.py      # ~1 min; needs /root/reference (build container only)

Data only, per configuration (all float64):
  cb{j}_*   the callback: `state0` [E,20] the initial states it drew, `actions` [T,E,6] what the stand-in policy's predict() returned at
            every step (recorded by wrapping the policy object, not the reference; NaN after an episode's end), `metrics` the 12 means.
  mc{j}_*   the Monte Carlo script on make_env(config=...): `rows` the indices into mc_initial_conditions.npz, `actions` [T,R,6],
            `table` [R,12] the 12 columns per row, `level` [R] the strictest constraint level a row ever reached (0: all four limits,
            1: three, 2: two, 3: one, -1: none — monte_carlo.py:163-184, read off the errors the script recorded).
  *_config_json   constructor arguments (cb: RendezvousEnv(**ctor); mc: make_env(config=config, stochastic=False)) and `assign`: limits
            given by attribute assignment, the way make_golden_thresholds.py passes parameters.

A replay of the recorded actions needs no policy.  The generator asserts that the fixture itself shows every branch the evaluators
have, and prints which configuration supplies it: no episode collides (-1), every episode collides, every episode starts inside the
keep-out zone (min pos error -1, first collision at t = 0), a mixed set, and all five strictest-level outcomes in the Monte Carlo rows.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import MC_COLUMNS, OUT, NumpyMlpPolicy, install_stubs, load_policy, state20   # noqa: E402
from make_golden_eval import METRICS                                                           # noqa: E402

RAD = float(np.radians(1))

# the callback: RendezvousEnv(**ctor), stochastic resets, `episodes` no multiple of 4
CALLBACK = [
    dict(name="dt0.5", ctor=dict(dt=0.5, t_max=30), assign={}, episodes=13, seed=311),
    dict(name="dt0.1", ctor=dict(dt=0.1, t_max=6), assign={}, episodes=27, seed=312),
    dict(name="all-collide", ctor=dict(koz_radius=9, corridor_half_angle=0.05, t_max=40), assign={}, episodes=13, seed=313),
    # 3 m beside the target, 90 deg off the corridor axis (45 deg of target attitude range leave it outside), chaser turned to face the target
    dict(name="start-in-koz", ctor=dict(rc0=[3.0, 0.0, 0.0], rc0_range=0, qc0=[float(np.sqrt(0.5)), 0.0, 0.0, float(np.sqrt(0.5))], t_max=40),
         assign={}, episodes=13, seed=314),
    dict(name="mixed", ctor=dict(dt=0.5, t_max=30, h=400e3, wt0=[0.0, 0.0, 2 * RAD], koz_radius=6), assign={}, episodes=27, seed=315),
]
# the Monte Carlo script: make_env(config=config, stochastic=False), 32 rows of the stored initial conditions
MONTE_CARLO = [
    dict(name="dt0.5", config=dict(dt=0.5, t_max=30), assign={}, rows=list(range(0, 32))),
    dict(name="dt0.1", config=dict(dt=0.1, t_max=6), assign={}, rows=list(range(32, 64))),
    dict(name="all-collide", config=dict(dt=1, t_max=40, koz_radius=9, corridor_half_angle=0.05), assign={}, rows=list(range(64, 96))),
    dict(name="sweep-axes", config=dict(dt=1, t_max=60, rc0=12, wt0=2 * RAD, h=400e3, koz_radius=6, corridor_half_angle=25 * RAD),
         assign={}, rows=list(range(96, 128))),
    dict(name="tight-limits", config=dict(dt=1, t_max=60), assign=dict(max_rd_error=0.2, max_vd_error=0.02, max_qd_error=1 * RAD,
                                                                        max_wd_error=0.2 * RAD), rows=list(range(128, 160))),
]


class RecordingPolicy:
    """The stand-in policy object with its predict() wrapped: every action it returns goes to the current episode's list."""

    def __init__(self, inner):
        self.inner, self.episodes = inner, []

    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        a, state = self.inner.predict(observation, state=state, episode_start=episode_start, deterministic=deterministic)
        self.episodes[-1].append(np.asarray(a, dtype=np.float64).copy())
        return a, state


def recording(env, model, tape):
    """env.reset() opens a new episode in the policy's record; the state it drew goes to `tape` (the callback: the start state)."""
    inner = env.reset

    def reset():
        obs = inner()
        tape.append(state20(env))
        model.episodes.append([])
        return obs
    env.reset = reset
    return env


def action_tape(episodes):
    T = max(len(e) for e in episodes)
    out = np.full((T, len(episodes), 6), np.nan)
    for i, e in enumerate(episodes):
        out[:len(e), i] = np.stack(e)
    return out


def with_arrays(kw):
    return {k: (np.array(v, dtype=np.float64) if isinstance(v, list) else v) for k, v in kw.items()}


def strictest_level(errors, env):
    """monte_carlo.py:159-184 on the error history the script itself would hold: 0 all four, 1 three, 2 two, 3 one, -1 none."""
    pos, vel, att, rot = errors.T
    pm, vm, am, rm = pos < env.max_rd_error, vel < env.max_vd_error, att < env.max_qd_error, rot < env.max_wd_error
    for level, mask in enumerate([pm & vm & am & rm, (pm & vm & am) | (pm & vm & rm), pm & vm, pm]):
        if mask.any():
            return level
    return -1


def main():
    install_stubs()
    cb_mod = types.ModuleType("stable_baselines3.common.callbacks")
    cb_mod.BaseCallback = object
    sys.modules["stable_baselines3.common.callbacks"] = cb_mod
    sys.modules["wandb"] = types.ModuleType("wandb")
    from rendezvous_env import RendezvousEnv
    from custom.custom_callbacks import CustomWandbCallback
    with contextlib.redirect_stdout(io.StringIO()):
        import monte_carlo
        from utils.environment_utils import make_env
    weights = load_policy()
    ics = np.load(os.path.join(OUT, "mc_initial_conditions.npz"))["states"]
    out, shows = {}, {k: [] for k in ("a", "b", "c", "d", "e")}
    out["cb_names"] = np.array([c["name"] for c in CALLBACK])
    out["mc_names"] = np.array([c["name"] for c in MONTE_CARLO])
    out["metric_names"] = np.array(METRICS)
    out["mc_columns"] = np.array(MC_COLUMNS)

    # ---- CustomWandbCallback.evaluate_policy
    for j, c in enumerate(CALLBACK):
        model, tape = RecordingPolicy(NumpyMlpPolicy(weights)), []
        env = RendezvousEnv(quiet=True, **with_arrays(c["ctor"]))
        for k, v in c["assign"].items():
            setattr(env, k, v)
        cb = object.__new__(CustomWandbCallback)
        cb.model, cb.n_evals, cb.env = model, c["episodes"], recording(env, model, tape)
        np.random.seed(c["seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            res = cb.evaluate_policy()
        actions = action_tape(model.episodes)
        assert len(tape) == c["episodes"] and c["episodes"] % 4 != 0 and actions.shape[0] <= 60, (c["name"], actions.shape)
        m = {k: float(res[k]) for k in METRICS}
        out[f"cb{j}_config_json"] = np.array(json.dumps(dict(ctor=c["ctor"], assign=c["assign"])))
        out[f"cb{j}_state0"] = np.stack(tape)
        out[f"cb{j}_actions"] = actions
        out[f"cb{j}_metrics"] = np.array([m[k] for k in METRICS])
        if env.dt in (0.5, 0.1):
            shows["a"].append(f"cb {c['name']} (dt {env.dt})")
        if m["ep_time_of_first_collision"] == -1 and m["%_collided_episodes"] == 0:
            shows["b"].append("cb " + c["name"])
        if m["%_collided_episodes"] == 100:
            shows["c"].append("cb " + c["name"])
        if m["ep_min_pos_error"] == -1 and m["ep_time_of_first_collision"] == 0:
            assert actions.shape[0] >= 10, "the episodes that start inside the KOZ should last (face the chaser to the target)"
            shows["d"].append("cb " + c["name"])
        if 0 < m["%_collided_episodes"] < 100:
            shows["e"].append(f"cb {c['name']} ({m['%_collided_episodes']:.1f} % collided)")
        print(f"cb{j} {c['name']}: {c['episodes']} episodes, {actions.shape[0]} steps at most;",
              {k: round(v, 4) for k, v in m.items()})

    # ---- monte_carlo.evaluate
    levels_seen = {}
    for j, c in enumerate(MONTE_CARLO):
        model, tape = RecordingPolicy(NumpyMlpPolicy(weights)), []
        with contextlib.redirect_stdout(io.StringIO()):
            env = make_env(reward_kwargs=None, quiet=True, config=dict(c["config"]), stochastic=False)
        for k, v in c["assign"].items():
            setattr(env, k, v)
        recording(env, model, tape)
        history = []                                   # the errors after every step: what monte_carlo.py:117, :140 record
        inner_step = env.step

        def step(a, inner_step=inner_step, env=env, history=history):
            r = inner_step(a)
            history[-1].append(np.asarray(env.get_errors(), dtype=np.float64))
            return r
        env.step = step
        table, level = [], []
        for i in c["rows"]:
            s = ics[i].copy()
            s[6:10] /= np.linalg.norm(s[6:10])         # monte_carlo.py:66-67
            s[13:17] /= np.linalg.norm(s[13:17])
            init = dict(rc=s[0:3], vc=s[3:6], qc=s[6:10], wc=s[10:13], qt=s[13:17], wt=s[17:20])
            history.append([])
            with contextlib.redirect_stdout(io.StringIO()):
                res = monte_carlo.evaluate(model, env, init)
            env.rc, env.vc, env.qc, env.wc, env.qt, env.wt = (init[k] for k in ("rc", "vc", "qc", "wc", "qt", "wt"))
            e0 = np.asarray(env.get_errors(), dtype=np.float64)          # the k = 0 sample (:117): the errors of the given state
            table.append([float(res[k]) for k in MC_COLUMNS])
            level.append(strictest_level(np.stack([e0] + history[-1]), env))
        actions = action_tape(model.episodes)
        assert len(model.episodes) == len(c["rows"]) == 32 and actions.shape[0] <= 60, (c["name"], actions.shape)
        table, level = np.array(table), np.array(level, dtype=np.float64)
        out[f"mc{j}_config_json"] = np.array(json.dumps(dict(config=c["config"], assign=c["assign"])))
        out[f"mc{j}_rows"] = np.array(c["rows"], dtype=np.float64)
        out[f"mc{j}_actions"] = actions
        out[f"mc{j}_table"] = table
        out[f"mc{j}_level"] = level
        for lv in np.unique(level):
            levels_seen.setdefault(int(lv), []).append(f"mc {c['name']} ({int((level == lv).sum())} rows)")
        if env.dt in (0.5, 0.1):
            shows["a"].append(f"mc {c['name']} (dt {env.dt})")
        print(f"mc{j} {c['name']}: {actions.shape[0]} steps at most, collided {int(table[:, 2].sum())}, succeeded {int(table[:, 6].sum())}, "
              f"strictest levels {dict(zip(*[x.tolist() for x in np.unique(level, return_counts=True)]))}")

    for k, what in (("a", "dt = 0.5 and dt = 0.1"), ("b", "no episode collides (-1)"), ("c", "every episode collides"),
                    ("d", "every episode starts inside the KOZ"), ("e", "a mixed set")):
        assert shows[k], f"no configuration shows branch {k}: {what}"
        print(f"branch {k} ({what}):", "; ".join(shows[k]))
    assert any("0.5" in s for s in shows["a"]) and any("0.1" in s for s in shows["a"])
    for lv, what in ((0, "all four limits"), (1, "three"), (2, "two"), (3, "one"), (-1, "no level reached")):
        assert lv in levels_seen, f"no Monte Carlo row whose strictest level is: {what}"
        print(f"branch f, strictest level = {what}:", "; ".join(levels_seen[lv]))
    assert all(v.dtype == np.float64 for k, v in out.items() if v.dtype.kind not in "US"), "float64 arrays only"
    path = os.path.join(OUT, "eval_reference_variants.npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""
What the GPU tests of the policy handles share (test_gpu_policy_mlp, test_gpu_policy_reference, test_gpu_policy_lstm,
test_gpu_policy_sets, test_gpu_lstm_policy_sets): the columns of a collect, the small device helpers, the env parameter sets and
staggered short episodes of the rollout tests, the loop rdv_rollout is defined by for a recurrent policy, rdv_policy_act with explicit
noise arguments, and THE comparison of a set's collect with its members' — ``assert_columns_equal``, which tests/test_policy_set_cases.py
shows can fail on every column.  A plain module, imported like policy_mlp_reference; torch is imported where it is used.
"""
import ctypes as C

import numpy as np

from helpers import to_numpy

DEV = "cuda:0"
COLUMNS = ("obs", "actions", "reward", "done", "log_prob", "last_obs", "values", "last_value", "advantages", "returns")


def starts(sizes):
    """the first row of every member"""
    return [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]


def close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def env_sets():
    """three parameter sets that differ in dt, KOZ radius, nominal state and t_max; 6, 8 and 6 steps to the time limit, so every env
    resets at least twice in 16 steps"""
    from reinforcement_learning_rendezvous_amd.params import make_params
    return [
        make_params(dt=1.0, t_max=6.0, koz_radius=5.0, rc0=np.array([0.5, -11.0, -0.3]), rc0_range=1.0, vc0_range=0.1,
                    wt0=np.radians([0.0, 0.0, 1.5]), wt0_range=np.radians(3.0)),
        make_params(dt=0.5, t_max=4.0, koz_radius=4.0, rc0=np.array([0.0, -2.2, 0.0]), rc0_range=1.5, vc0_range=0.05,
                    qt0_range=np.radians(60.0), wt0=np.radians([1.0, -2.0, 0.5]), wt0_range=np.radians(1.0)),
        make_params(dt=2.0, t_max=12.0, koz_radius=3.5, rc0=np.array([-1.0, -18.0, 2.0]), rc0_range=2.0, vc0_range=0.2,
                    wt0=np.radians([-2.0, 0.5, 0.0]), wt0_range=np.radians(4.0)),
    ]


def short_episodes():
    from reinforcement_learning_rendezvous_amd.params import make_params
    return make_params(dt=1.0, t_max=4.0)


def stagger(env):
    """Four steps with zero actions, rows r % 5 > s reset behind step s: five episode ages, so that with episodes of 4 steps some
    envs, never all, finish at every step of the rollouts that follow (60 or 120 of 300; counted on the CPU oracle)."""
    import torch
    n = env.num_envs
    zero = torch.zeros((n, 6), dtype=torch.float32, device=DEV)
    r = torch.arange(n, device=DEV)
    for s in range(4):
        env.step(zero)
        env.reset(mask=(r % 5 > s))


def lstm_loop(env, pol, T, ctr0):
    """The loop rdv_rollout is defined by, through the Python calls: rdv_lstm_act(flags) on the policy or the set + rdv_step.
    Returns (the rows, the flags behind the last step)."""
    import torch
    n = env.num_envs
    rows = dict(obs=[], actions=[], reward=[], done=[], log_prob=[])
    obs = env.obs.clone()
    flags = pol._pending_flags("l", torch.device(DEV))
    for t in range(T):
        raw = torch.empty((n, 6), dtype=torch.float32, device=DEV)
        lp = torch.empty((n,), dtype=torch.float32, device=DEV)
        pol._calls = ctr0 + t
        act = pol.act(obs, episode_start=flags, deterministic=False, env_id_offset=env.env_id_offset, raw_out=raw, log_prob_out=lp)
        o, r, d = env.step(act)
        rows["obs"].append(obs); rows["actions"].append(raw); rows["reward"].append(r.clone()); rows["done"].append(d.clone().to(torch.uint8)); rows["log_prob"].append(lp)
        obs, flags = o.clone(), d.clone().to(torch.uint8)
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["last_obs"] = obs
    return out, flags


def act_via_abi(handle, obs, deterministic=True, seed=0, counter=0, offset=0):
    """rdv_policy_act through the C ABI with every noise argument given explicitly: obs (a device tensor, or an array for ``dev``) ->
    the actions on the device, every entry preset to 7."""
    import torch
    from reinforcement_learning_rendezvous_amd import _native as N
    o = obs if torch.is_tensor(obs) else dev(obs)
    out = torch.full((o.shape[0], 6), 7.0, dtype=torch.float32, device=DEV)
    N.check(N.lib().rdv_policy_act(handle, C.c_void_p(o.data_ptr()), C.c_void_p(out.data_ptr()), o.shape[0], int(deterministic),
                                   C.c_uint64(seed), C.c_uint64(counter), C.c_uint64(offset),
                                   C.c_void_p(torch.cuda.current_stream(o.device).cuda_stream)))
    return out


def assert_columns_equal(got, want_parts, what, extra=()):
    """A set's collect ``got`` (a dict of tensors) against its members' ``want_parts`` (one dict per member, in member order): every
    column of COLUMNS equals the members' concatenated over the env axis (axis 0 of last_obs and last_value, axis 1 of the [T, N, ...]
    columns), by equality; with ``extra=("lstm_state0",)`` so do both halves (h, c: [N, H]) of the state at the rollout's start.  A
    failure names the column."""
    import torch
    for name in COLUMNS:
        axis = 0 if name in ("last_obs", "last_value") else 1
        np.testing.assert_array_equal(to_numpy(got[name]), np.concatenate([to_numpy(w[name]) for w in want_parts], axis=axis),
                                      err_msg=f"{name}, {what}")
    for name in extra:
        for i, half in enumerate("hc"):
            assert torch.equal(got[name][i], torch.cat([w[name][i] for w in want_parts], dim=0)), f"{name} {half}, {what}"

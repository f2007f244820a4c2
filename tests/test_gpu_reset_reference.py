"""
GPU tests (run with `-m gpu`): every place that computes a Philox reset, against the reference's own reset().

tests/golden/reset_reference.npz holds what the UNMODIFIED RendezvousEnv.reset() returns for the uniforms of (seed, global env id,
episode) — 7 parameter sets x episodes 0, 1, 2 x 160 consecutive ids that cross 2^32 (both counter words of the stream change inside
the batch; the seed's high word is not zero).  In every set but the defaults the nominal attitudes are rotated and not of unit length
and the nominal body rates are not zero, so the factor order and cross-term signs of the quaternion product, the normalisation of the
nominal and the R(q)^T w rotations do not cancel; (c) starts at the docking port (collided and successful initial states), (e) and (f)
sit on the switch between the two cos / sinc series, (g) draws both attitudes from the whole sphere.  The comparison is with the
golden directly, not with the oracle (which tests/test_oracle_golden.py pins to the same file).

Covered, each with the kernel's name asserted (rdv_debug_last_kernel against tests/helpers.py):
  rdv_reset (reset_kernel: whole and masked); the in-kernel reset of step_kernel_parts (fused, and auto above 65,536 envs, golden ids in
  the ragged last wave), step_kernel_split, step_kernel<ST, false> (in-lane), step_kernel_tiles, the evaluator build step_kernel<ST, true>,
  the general-body kernels step_kernel_general and step_kernel<ST, false, true>; the prepared-state slots of step_many_kernel and
  rollout_kernel (whole refill by reset_kernel / prepare_kernel, refill by part, flags evaluated by the taker in set (c)).

Tolerances.
  fp64 storage: max |GPU - golden| / max(1, |x|), printed per check before it is asserted.  The differences come from rsqrt64, the
  truncated series and FMA contraction.  Asserted: 8 x the largest value observed on an MI355X, not below 16 eps = 3.6e-15 (FP64_BOUND),
  never above the project's state tolerance 1e-10.  NOT MEASURED YET: this module has not run on an MI355X, so FP64_OBSERVED is 0 and
  the bound is its floor, 16 eps (the CPU oracle, which does the same fp64 operations without the kernel's shortcuts, is within
  1.1e-16 of the same golden).  The first GPU run prints the figures; they belong here and in DESIGN.md section 3, item 9.
  f32 storage: the stored value is within one float32 ulp of float32(golden) (the fp64 error is far below half an ulp: the two roundings
  differ only next to a tie; the number of entries that differ at all is printed).
  Observations: the project's reset-observation tolerance (tests/parity.py, RESET_OBS_TOL).
  collided / success: exact in fp64 storage; in f32 storage exact on the rows whose flag decisions have a margin in the reference's own
  numbers (flags_robust), and on all rows equal to the oracle's f32-storage flags.
"""
import numpy as np
import pytest

import oracle
import parity
from helpers import counter_actions, expected_kernel, gpu_batch, persistent_kernel, shipped_policy, to_numpy
from test_oracle_golden import RESET_SETS, load_reset_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
FP64_OBSERVED = 0.0                                       # largest value observed on an MI355X (none yet: see the docstring)
FP64_BOUND = max(16 * EPS, 8 * FP64_OBSERVED)
assert FP64_BOUND <= 1e-10
STORAGES = ["f64", "f32"]


_cache = {}


def _golden(name):
    """The set's golden, plus the oracle's flags with float32 state storage (what the f32 kernels must give on every row)."""
    if name not in _cache:
        g = load_reset_golden(name)
        ob = oracle.OracleBatch(g["n"], g["oracle_params"], storage=oracle.STORAGE_F32, seed=g["seed"], env_id_offset=g["env_id_offset"])
        flags = []
        for _ in range(g["state"].shape[0]):
            ob.reset()
            flags.append(ob.get_aux()[:, [2, 3]].copy())
        g["oracle_f32_flags"] = np.stack(flags)
        _cache[name] = g
    return _cache[name]


def _every_step_ends(p):
    """The shortest episode rdv_params_validate admits: t_max = dt, every env finishes on every step (reset() does not depend on either)."""
    q = p.copy()
    q.t_max = q.dt
    return q


def check_state(state, g, episode, storage, what, rows=None):
    """state [n,20] (float64 as rdv_get_state returns it) against golden episode `episode` (an int, or one per row)."""
    rows = np.arange(g["n"]) if rows is None else np.asarray(rows)
    ep = np.broadcast_to(np.asarray(episode), rows.shape)
    want = g["state"][ep, rows]
    assert state.shape == want.shape, (what, state.shape, want.shape)
    if storage == "f64":
        err = np.abs(state - want) / np.maximum(1.0, np.abs(want))
        worst = float(err.max()) if err.size else 0.0
        print(f"{what}: fp64 state, max |GPU - golden| / max(1, |x|) = {worst:.3e} (bound {FP64_BOUND:.3e})")
        assert worst <= FP64_BOUND, (what, worst, np.argwhere(err > FP64_BOUND)[:5].tolist())
    else:
        want32 = want.astype(np.float32)
        got32 = state.astype(np.float32)
        assert np.array_equal(got32.astype(np.float64), state), f"{what}: f32 storage returned values that are not float32"
        diff = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
        ulp = np.spacing(np.abs(want32)).astype(np.float64)
        print(f"{what}: f32 state, {int((diff > 0).sum())} of {diff.size} entries differ from float32(golden)")
        assert (diff <= ulp).all(), (what, np.argwhere(diff > ulp)[:5].tolist())


def check_obs(obs, g, episode, what, rows=None):
    rows = np.arange(g["n"]) if rows is None else np.asarray(rows)
    ep = np.broadcast_to(np.asarray(episode), rows.shape)
    parity.check_reset_obs(obs, g["obs"][ep, rows], f"{what}: obs")


def check_flags(aux, g, episode, storage, what, rows=None, counter=True):
    """aux [n,8] of rdv_get_aux: collided, success (columns 2, 3) and the episode counter (column 7: episodes started)."""
    rows = np.arange(g["n"]) if rows is None else np.asarray(rows)
    ep = np.broadcast_to(np.asarray(episode), rows.shape)
    want = np.stack([g["collided"][ep, rows], g["success"][ep, rows]], axis=1).astype(np.float64)
    if storage == "f64":
        np.testing.assert_array_equal(aux[:, [2, 3]], want, err_msg=f"{what}: collided / success")
    else:
        ok = g["flags_robust"][ep, rows]
        np.testing.assert_array_equal(aux[ok][:, [2, 3]], want[ok], err_msg=f"{what}: collided / success on the robust rows")
        np.testing.assert_array_equal(aux[:, [2, 3]], g["oracle_f32_flags"][ep, rows], err_msg=f"{what}: collided / success vs the f32 oracle")
    if counter:
        np.testing.assert_array_equal(aux[:, 7], ep + 1, err_msg=f"{what}: episode counter")


def check_all(env, obs, g, episode, storage, what, rows=None, tail=None):
    """obs, rdv_get_state and rdv_get_aux of `env` (its last `tail` rows, when it is larger than the golden) against one golden episode."""
    sl = slice(None) if tail is None else slice(env.num_envs - tail, env.num_envs)
    pick = (lambda x: x[sl]) if rows is None else (lambda x: x[sl][rows])
    check_obs(pick(to_numpy(obs)), g, episode, what, rows)
    check_state(pick(to_numpy(env.get_state())), g, episode, storage, what, rows)
    check_flags(pick(to_numpy(env.get_aux())), g, episode, storage, what, rows)


# ------------------------------------------------------------------------------------------------------- rdv_reset
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", RESET_SETS)
def test_cold_reset_kernel(name, storage):
    """rdv_reset three times over: episodes 0, 1, 2.  Then a masked reset of alternate rows of a fresh batch: those move on to episode 1,
    the others keep their episode-0 state and their episode counter."""
    g = _golden(name)
    env = gpu_batch(g["n"], params=g["params"], storage=storage, seed=g["seed"], env_id_offset=g["env_id_offset"])
    for e in range(3):
        check_all(env, env.reset(), g, e, storage, f"{name}: reset_kernel, episode {e}")
    assert env.last_kernel == ""                     # no step kernel has run: these states are reset_kernel's
    env.close()
    env = gpu_batch(g["n"], params=g["params"], storage=storage, seed=g["seed"], env_id_offset=g["env_id_offset"])
    env.reset()
    mask = (np.arange(g["n"]) % 2 == 1)
    obs = env.reset(torch.from_numpy(mask.astype(np.uint8)).cuda())
    episode = mask.astype(np.int64)
    check_all(env, obs, g, episode, storage, f"{name}: reset_kernel, masked")
    env.close()


# ------------------------------------------------------------------------------------------------------- the reset inside rdv_step
def _auto_reset_run(g, name, storage, variant, n=None, diag=False, body=None, kernel=None):
    n_gold = g["n"]
    n = n_gold if n is None else n
    offset = g["env_id_offset"] - (n - n_gold)                      # the golden ids are the LAST 160 rows
    env = gpu_batch(n, params=_every_step_ends(g["params"]), storage=storage, seed=g["seed"], env_id_offset=offset, variant=variant)
    if body:
        env.set_rigid_body(**body)
    tail = None if n == n_gold else n_gold
    who = f"{name}: {kernel or variant}{' diag' if diag else ''} n={n}"
    check_all(env, env.reset(), g, 0, storage, f"{who}, reset_kernel", tail=tail)
    zero = torch.zeros((n, 6), dtype=torch.float32, device="cuda:0")
    want_kernel = kernel or expected_kernel(variant, n, storage, "reset", diag=diag)
    for e in (1, 2):
        obs, _, done = env.step(zero, diag=diag)
        assert env.last_kernel == want_kernel, f"{who}: ran {env.last_kernel!r}, expected {want_kernel!r}"
        assert to_numpy(done).all(), f"{who}: every env finishes on every step"
        check_all(env, obs, g, e, storage, f"{who}, episode {e}", tail=tail)
    env.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("variant", ["fused", "split", "fused_inlane", "fused_tiles", "evaluator"])
@pytest.mark.parametrize("name", RESET_SETS)
def test_auto_reset_in_the_step_kernels(name, variant, storage):
    """on_done = reset, zero actions, t_max = dt: after each step every env holds the initial state of its next episode."""
    g = _golden(name)
    if variant == "evaluator":
        _auto_reset_run(g, name, storage, "auto", diag=True)
    else:
        _auto_reset_run(g, name, storage, variant)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", RESET_SETS)
def test_auto_reset_above_the_split_limit(name, storage):
    """auto with 65,536 + 77 envs runs step_kernel_parts; env_id_offset puts the golden ids on the last 160 rows, which end in a ragged
    wave of the ragged last workgroup (and start in the middle of a wave)."""
    _auto_reset_run(_golden(name), name, storage, "auto", n=65536 + 77)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", RESET_SETS)
def test_auto_reset_in_the_general_body_kernels(name, storage):
    """reset() does not depend on the bodies: a tri-axial target (step_kernel_general: the target integrates on partner waves) and a
    tri-axial chaser beside the reference's target (the fused per-lane form) give the same initial states."""
    g = _golden(name)
    st = "float" if storage == "f32" else "double"
    _auto_reset_run(g, name, storage, "auto", body=dict(inertia_target=[9.0, 16.0, 27.0]), kernel=f"step_kernel_general<{st}>")
    _auto_reset_run(g, name, storage, "auto", body=dict(inertia=[10.0, 20.0, 30.0]), kernel=f"step_kernel<{st}, false, true>")


# ------------------------------------------------------------------------------------------------------- the prepared-state slots
def _episode_after(done):
    """done [T,N] -> the episode each env is in AFTER step t (the number of episodes it has finished so far)."""
    return np.cumsum(done.astype(np.int64), axis=0)


def _check_reset_rows(obs_after, done, g, what):
    """Among the rows obs_after[t] (the observation after step t) those of envs that finished at step t are reset observations: of
    episode _episode_after(done)[t], compared where the golden has it.  Returns the number of rows compared."""
    ep = _episode_after(done)
    seen = 0
    for t in range(done.shape[0]):
        rows = np.flatnonzero((done[t] != 0) & (ep[t] <= 2))
        if rows.size:
            check_obs(obs_after[t][rows], g, ep[t][rows], f"{what}, step {t}", rows)
            seen += rows.size
    return seen


def _check_final(env, done, g, storage, what):
    """After the launch: the envs that finished on the LAST step hold a fresh initial state."""
    ep = _episode_after(done)[-1]
    rows = np.flatnonzero((done[-1] != 0) & (ep <= 2))
    assert rows.size >= g["n"] // 2, (what, rows.size)
    check_state(to_numpy(env.get_state())[rows], g, ep[rows], storage, what, rows)
    check_flags(to_numpy(env.get_aux())[rows], g, ep[rows], storage, what, rows)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", RESET_SETS)
def test_step_many_takes_and_refills_the_slots(name, storage):
    """rdv_step_many: an env whose episode ends copies its prepared slot.  Three ways a slot comes to hold its state:
      t_max = dt, K = 2 after rdv_reset: episode 1 from the slot reset_kernel filled (whole), episode 2 refilled by part inside the launch;
      a rdv_step in between (the slots lag behind, prepare_kernel re-derives them), then K = 1: episode 2 from prepare_kernel's slot;
      t_max = 2 dt, K = 4: envs end their episodes at different steps (attitude, bubble), two time-outs for those that last.
    In set (c) the rc + vc part finds the state close to the target and leaves the flags to the lane that takes the slot."""
    g = _golden(name)
    n = g["n"]
    mk = lambda p: gpu_batch(n, params=p, storage=storage, seed=g["seed"], env_id_offset=g["env_id_offset"])
    kernel = persistent_kernel("step_many", storage)
    tape = lambda k0, K: torch.from_numpy(np.stack([0.5 * counter_actions(11, k0 + k, n) for k in range(K)])).cuda()

    env = mk(_every_step_ends(g["params"]))
    env.reset()
    out = env.step_many(tape(0, 2))
    assert env.last_kernel == kernel, env.last_kernel
    done = to_numpy(out["done"])
    assert done.all()
    assert _check_reset_rows(to_numpy(out["obs"]), done, g, f"{name}: step_many") == 2 * n
    _check_final(env, done, g, storage, f"{name}: step_many, final")
    env.close()

    env = mk(_every_step_ends(g["params"]))
    env.reset()
    env.step(tape(0, 1)[0])                                          # rdv_step resets in registers: episode 1, the slots are stale
    assert env.last_kernel == expected_kernel("auto", n, storage, "reset")
    out = env.step_many(tape(1, 1))
    assert env.last_kernel == kernel, env.last_kernel
    check_all(env, out["obs"][0], g, 2, storage, f"{name}: step_many after rdv_step")
    env.close()

    p = g["params"].copy()
    p.t_max = 2 * p.dt
    env = mk(p)
    env.reset()
    out = env.step_many(tape(0, 4))
    assert env.last_kernel == kernel, env.last_kernel
    done = to_numpy(out["done"])
    assert _check_reset_rows(to_numpy(out["obs"]), done, g, f"{name}: step_many, t_max = 2 dt") >= 2 * n
    env.close()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", RESET_SETS)
def test_rollout_takes_and_refills_the_slots(name, storage):
    """rdv_rollout with the shipped policy, deterministic: obs[t] is what the actor saw, so the row after a finished step is a reset
    observation.  t_max = dt, T = 2 (episodes 0, 1, 2 in obs[0], obs[1], last_obs) and t_max = 2 dt, T = 4."""
    g = _golden(name)
    n = g["n"]
    kernel = persistent_kernel("rollout", storage)
    pol = shipped_policy("cuda:0")

    env = gpu_batch(n, params=_every_step_ends(g["params"]), storage=storage, seed=g["seed"], env_id_offset=g["env_id_offset"])
    env.reset()
    ro = env.rollout(pol, 2, deterministic=True)
    assert env.last_kernel == kernel, env.last_kernel
    done = to_numpy(ro["done"])
    assert done.all()
    check_obs(to_numpy(ro["obs"][0]), g, 0, f"{name}: rollout, obs[0]")
    after = np.concatenate([to_numpy(ro["obs"])[1:], to_numpy(ro["last_obs"])[None]])       # the observation AFTER step t
    assert _check_reset_rows(after, done, g, f"{name}: rollout") == 2 * n
    _check_final(env, done, g, storage, f"{name}: rollout, final")
    env.close()

    p = g["params"].copy()
    p.t_max = 2 * p.dt
    env = gpu_batch(n, params=p, storage=storage, seed=g["seed"], env_id_offset=g["env_id_offset"])
    env.reset()
    ro = env.rollout(pol, 4, deterministic=True)
    assert env.last_kernel == kernel, env.last_kernel
    done = to_numpy(ro["done"])
    after = np.concatenate([to_numpy(ro["obs"])[1:], to_numpy(ro["last_obs"])[None]])
    assert _check_reset_rows(after, done, g, f"{name}: rollout, t_max = 2 dt") >= 2 * n
    env.close()
    pol.close()

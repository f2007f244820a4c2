"""
GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI, against
  (1) the golden transition tuples recorded from the unmodified reference (tests/golden/steps_*.npz), in fp64 storage, and
  (2) the CPU oracle on identical (seed, action) sequences, in both storage precisions.

What is compared, at which tolerance and why: tests/parity.py (the step comparison against the oracle, and the golden replay; the
numbers of the golden replay in fp64 storage are passed below).
"""
import numpy as np
import pytest

import parity
from helpers import counter_actions, gpu_batch, load_golden, oracle_batch, params_from_note, to_numpy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCENARIOS = ["A_random", "B_mc_policy", "C_variant", "D_stochastic", "E_spin"]

# Every variant runs the TRAINING path (no diag / eval outputs), so that it really launches its own kernel: a step with diag=True runs
# the evaluator build step_kernel<ST, true> whatever the variant.  Each scenario and storage then has exactly one evaluator pass of
# its own (the *_evaluator_build tests).  With a reset tape or in halt mode "fused_tiles" runs step_kernel_parts (include/rdv.h): those
# cases assert that fallback through last_kernel.
VARIANTS = ["fused", "split", "fused_inlane", "fused_tiles"]


def _golden_run(name, variant, diag):
    g = load_golden(f"steps_{name}.npz")
    p, _ = params_from_note(g["env_kwargs_json"])
    halt = name.startswith("B")
    env = gpu_batch(g["actions"].shape[1], params=p, storage="f64", on_done="halt" if halt else "reset", variant=variant)
    # fp64 storage against the reference's own fp64 records: observations to 1 float32 ulp, the float32 reward to 2e-7
    parity.replay_golden(env, g, halt=halt, diag=diag, variant=variant, obs_tol=1.2e-7, reward_kw=dict(rtol=2e-7, atol=2e-7))
    env.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SCENARIOS)
def test_golden_transitions_fp64_storage(name, variant):
    """HIP kernel (parity mode, training path) vs the reference's own recorded transitions.  B runs in halt mode from set_state:
    its first step is the kRaw kernel, the rest the variant's own."""
    _golden_run(name, variant, diag=False)


@pytest.mark.parametrize("name", SCENARIOS)
def test_golden_transitions_fp64_storage_evaluator_build(name):
    """The evaluator build (diag outputs) vs the reference's recorded transitions and its evaluator helpers."""
    _golden_run(name, "auto", diag=True)


def _golden_vs_oracle(name, storage, variant):
    g = load_golden(f"steps_{name}.npz")
    p, _ = params_from_note(g["env_kwargs_json"])
    T, E = g["actions"].shape[:2]
    tape = np.nan_to_num(g["tape"])
    env = gpu_batch(E, params=p, storage=storage, variant=variant)
    env.set_reset_tape(torch.from_numpy(tape))
    orc = oracle_batch(E, p, storage, tape=tape)
    np.testing.assert_array_equal(to_numpy(env.reset()), orc.reset())
    return env, orc, [g["actions"][t] for t in range(T)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("name", ["A_random", "C_variant", "D_stochastic"])
def test_golden_actions_vs_oracle(name, storage, variant):
    """Same tapes and action sequences, HIP (training path) vs oracle in the same storage precision (covers fp32 production mode)."""
    env, orc, actions = _golden_vs_oracle(name, storage, variant)
    parity.run_against_oracle(env, orc, actions, storage, variant, tape=True)


# The evaluator passes of this module compare the flags of the diag output, not its error norms (diag_errors=False): their set as
# it has always been.
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("name", ["A_random", "C_variant", "D_stochastic"])
def test_golden_actions_vs_oracle_evaluator_build(name, storage):
    env, orc, actions = _golden_vs_oracle(name, storage, "auto")
    parity.run_against_oracle(env, orc, actions, storage, "auto", evaluator=True, diag_errors=False)


def _config2(storage, variant):
    n = 4096
    env = gpu_batch(n, storage=storage, seed=0, variant=variant)
    orc = oracle_batch(n, env.params, storage, seed=0, n_threads=8)
    np.testing.assert_array_equal(to_numpy(env.reset()), orc.reset())
    return env, orc, [counter_actions(1, t, n) for t in range(512)]


# config 2 compares the outputs on every step, diag / state / aux on every 16th (512 steps of 4096 envs on the CPU oracle)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_config2_4096x512_random_actions_philox_resets(storage, variant):
    """BASELINE config 2: 4096 envs x 512 steps, U(-1,1) actions keyed by (seed, step, env), in-kernel Philox resets, on the
    variant's own kernel (the training path)."""
    env, orc, actions = _config2(storage, variant)
    parity.run_against_oracle(env, orc, actions, storage, variant, diag_every=16, state_every=16)
    assert env.get_stats()["episodes"] > 50_000     # ~5 % of envs end per step (bubble)


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_config2_4096x512_random_actions_philox_resets_evaluator_build(storage):
    env, orc, actions = _config2(storage, "auto")
    parity.run_against_oracle(env, orc, actions, storage, "auto", evaluator=True, diag_errors=False, diag_every=16, state_every=16)
    assert env.get_stats()["episodes"] > 50_000


def _ragged(variant, diag):
    for n in (1, 63, 65, 129, 257, 1000):
        env = gpu_batch(n, storage="f32", seed=11, variant=variant)
        orc = oracle_batch(n, env.params, "f32", seed=11)
        np.testing.assert_array_equal(to_numpy(env.reset()), orc.reset())
        kw = dict(evaluator=True, diag_errors=False) if diag else {}
        parity.run_against_oracle(env, orc, [counter_actions(5, t, n) for t in range(40)], "f32", variant, **kw)
        mask = (np.arange(n) % 3 == 0).astype(np.uint8)
        np.testing.assert_allclose(to_numpy(env.reset(torch.from_numpy(mask))), orc.reset(mask), rtol=0, atol=parity.OBS_TOL)
        parity.run_against_oracle(env, orc, [counter_actions(6, t, n) for t in range(10)], "f32", variant, **kw)
        env.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_ragged_sizes_and_masked_reset(variant):
    """N not a multiple of the wave / block size, single env, and reset(mask)."""
    _ragged(variant, diag=False)


def test_ragged_sizes_and_masked_reset_evaluator_build():
    _ragged("auto", diag=True)


def test_sharding_is_index_independent():
    """Env i of a shard with env_id_offset=o behaves exactly as env o+i of the unsharded batch (RNG keyed by global id),
    and the two kernel variants give bit-identical outputs."""
    n = 512
    full = gpu_batch(n, storage="f32", seed=5, variant="fused")
    lo = gpu_batch(n // 2, storage="f32", seed=5, env_id_offset=0, variant="split")
    hi = gpu_batch(n // 2, storage="f32", seed=5, env_id_offset=n // 2, variant="split")
    o = to_numpy(full.reset())
    np.testing.assert_array_equal(o[: n // 2], to_numpy(lo.reset()))
    np.testing.assert_array_equal(o[n // 2:], to_numpy(hi.reset()))
    for t in range(64):
        a = counter_actions(2, t, n)
        of, rf, df = [to_numpy(x).copy() for x in full.step(torch.from_numpy(a).cuda())]
        ol, rl, dl = [to_numpy(x) for x in lo.step(torch.from_numpy(a[: n // 2]).cuda())]
        oh, rh, dh = [to_numpy(x) for x in hi.step(torch.from_numpy(a[n // 2:]).cuda())]
        np.testing.assert_array_equal(of, np.concatenate([ol, oh]))
        np.testing.assert_array_equal(rf, np.concatenate([rl, rh]))
        np.testing.assert_array_equal(df, np.concatenate([dl, dh]))


def test_errors_are_loud():
    from reinforcement_learning_rendezvous_amd import RdvError
    env = gpu_batch(8)
    with pytest.raises(RdvError):
        env.step(torch.zeros((8, 6), device="cuda:0"))           # step before reset: state undefined (reference :44-49)
    env.reset()
    with pytest.raises(ValueError):
        env.step(torch.zeros((8, 5), device="cuda:0"))           # reference asserts action.shape == (6,) (:168)
    with pytest.raises(ValueError):
        env.step(torch.zeros((8, 6), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(RdvError):
        gpu_batch(0)
    with pytest.raises(AssertionError):
        gpu_batch(4, koz_radius=1.5)                                 # reference assert :155


def test_verification_script_scenarios_on_the_gpu():
    """The known answers of the reference's verification/ scripts (tests/test_oracle_golden.py has them for
    the oracle), through the HIP path with ``on_done="continue"`` — those scripts ignore `done` and keep stepping the env object."""
    import oracle
    from reinforcement_learning_rendezvous_amd.batch import RendezvousBatch
    from reinforcement_learning_rendezvous_amd.params import make_params
    quiet = dict(rc0_range=0, vc0_range=0, qc0_range=0, wc0_range=0, qt0_range=0, wt0_range=0)
    zero = torch.zeros((64, 6), device="cuda:0")
    # KAT-1 verification/verify_cw.py:12-74: K zero-action steps == one closed-form CW propagation over K*dt
    p = make_params(**quiet)
    s = np.array([0.3, -9.0, 0.2, 0.01, -0.02, 0.005, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0.0])
    env = RendezvousBatch(64, params=p, device="cuda:0", storage="f64", on_done="continue")
    env.reset(); env.set_state(torch.from_numpy(np.tile(s, (64, 1))))
    n_done = 0
    for _ in range(200):
        _, _, d = env.step(zero)
        n_done += int(d[0])
    r, v = oracle.cw_solution(s[0:3], s[3:6], p.n, 200 * p.dt)
    st = env.get_state().cpu().numpy()
    np.testing.assert_allclose(st[:, 0:3], np.tile(r, (64, 1)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(st[:, 3:6], np.tile(v, (64, 1)), rtol=0, atol=1e-12)
    assert n_done > 50 and float(env.get_aux()[0, 0]) == 200.0          # done was reported (t >= t_max = 120 s) and ignored
    env.close()
    # KAT-4 verification/verify_attitude_torque.py:34-60: action [0,0,0,0,0,0.5], dt = 0.5, 65 steps -> w_z = 0.195 rad/s
    p = make_params(dt=0.5, **quiet)
    env = RendezvousBatch(64, params=p, device="cuda:0", storage="f64", on_done="continue")
    env.reset()
    a = torch.zeros((64, 6), device="cuda:0"); a[:, 5] = 0.5
    for _ in range(65):
        env.step(a)
    st = env.get_state().cpu().numpy()
    assert st[0, 12] == pytest.approx(0.195, rel=1e-9) and np.abs(np.linalg.norm(st[:, 6:10], axis=1) - 1).max() < 1e-15
    env.close()
    # KAT-5 verification/verify_attitude_racket.py:34-45: the env's isotropic body -> rate constant over 760 s, |q| = 1
    p = make_params(**quiet)
    s = np.zeros(20); s[1] = -10; s[6] = 1; s[13] = 1; s[10:13] = np.radians([0, 5, 0.01])
    env = RendezvousBatch(64, params=p, device="cuda:0", storage="f64", on_done="continue")
    env.reset(); env.set_state(torch.from_numpy(np.tile(s, (64, 1))))
    for _ in range(760):
        env.step(zero)
    st = env.get_state().cpu().numpy()
    np.testing.assert_array_equal(st[:, 10:13], np.tile(s[10:13], (64, 1)))
    assert np.abs(np.linalg.norm(st[:, 6:10], axis=1) - 1).max() < 1e-15
    # ... and with a tri-axial body the same start does flip about the intermediate axis (the effect the script was written to show)
    env.set_rigid_body(inertia=[10.0, 20.0, 30.0])
    env.set_state(torch.from_numpy(np.tile(s, (64, 1))))
    wy = []
    for _ in range(760):
        env.step(zero)
        wy.append(float(env.get_state()[0, 11]))
    assert min(wy) < -0.9 * s[11] and max(wy) > 0.9 * s[11]             # w_y changes sign: Dzhanibekov flips
    env.close()


def test_snapshot_restore_resumes_bit_for_bit():
    """rdv_snapshot / rdv_restore: the whole batch (state, flags, episode counters = reset RNG position, statistics)."""
    from reinforcement_learning_rendezvous_amd.batch import RendezvousBatch
    n = 1500
    for on_done in ("reset", "halt"):
        env = RendezvousBatch(n, device="cuda:0", storage="f32", on_done=on_done, seed=13)
        env.reset()
        acts = [torch.from_numpy(counter_actions(8, t, n)).cuda() for t in range(40)]
        for t in range(15):
            env.step(acts[t])
        snap = env.snapshot()
        stats0 = env.get_stats()
        first = [tuple(x.clone() for x in env.step(acts[t])) for t in range(15, 40)]
        state1, stats1 = env.get_state().clone(), env.get_stats()
        env.restore(snap)
        assert env.get_stats() == stats0
        for t in range(15, 40):
            o, r, d = env.step(acts[t])
            assert torch.equal(o, first[t - 15][0]) and torch.equal(r, first[t - 15][1]) and torch.equal(d, first[t - 15][2]), t
        assert torch.equal(env.get_state(), state1) and env.get_stats() == stats1
        other = RendezvousBatch(n, device="cuda:0", storage="f32", on_done=on_done, seed=13)     # a fresh handle takes it too
        other.restore(snap)
        o, r, d = other.step(acts[15])
        assert torch.equal(o, first[0][0]) and torch.equal(d, first[0][2])
        with pytest.raises(ValueError):
            RendezvousBatch(2 * n, device="cuda:0", storage="f32").restore(snap)
        env.close(); other.close()

"""What "parity" means in this suite: one RendezvousBatch.step against one OracleBatch.step, stated once.

Arithmetic is fp64 on both sides; the device uses fused multiply-adds and its own libm, the oracle neither, so agreement is to a few
fp64 ulps per step, not bitwise.  Everything the reference compares (done, reasons, flags, counters) is exact.  The functions take
anything with the engine surface of RendezvousBatch (tests/oracle_engine.py::OracleEngine has it, which is how
tests/test_parity_helpers.py proves on the CPU that every check below can fail).  A call site whose number differs from a constant
here passes it by keyword and says so in a comment.
"""
import numpy as np

from helpers import batch_modes, expect_kernel, to_numpy

OBS_TOL = 2.4e-7               # absolute: 2 float32 ulps of an observation in [-1, 1] (f32 storage re-rounds the state every step)
RESET_OBS_TOL = 1.2e-7         # absolute: 1 float32 ulp, no step arithmetic behind a reset observation
REWARD_TOL = 2e-6              # relative and absolute: the reward is a float32 output of fp64 sums over a re-rounded state
STATE_TOL = {"f32": 2.5e-7,    # relative to max(1, |x|): 2 float32 ulps, the two roundings differ only next to a tie
             "f64": 1e-10}     # a few fp64 ulps per step, accumulated over an episode
AUX_TOL = 1e-5                 # relative and absolute: bubble radius, delta-v / delta-w sums, kept in the storage precision
DIAG_TOL = 1e-6                # relative and absolute: error norms derived from the (f32: re-rounded) state
RETURN_TOL = 1e-5              # relative and absolute: a float32 sum of up to t_max / dt rewards
STATS_SUM_TOL = 1e-5           # relative to max(1, |sum|): fp64 sums of float32 terms in another order

DIAG_FLAGS, DIAG_ERRORS = [4, 5, 7], [0, 1, 2, 3, 6]   # collided, success, entered the KOZ | pos, vel, att, rot errors, distance from the KOZ
AUX_EXACT, AUX_REAL = [0, 2, 3, 7], [1, 4, 5, 6]       # t, collided, success count, episode index | bubble radius, delta-v, delta-w, return
STATS_COUNTERS = ("env_steps", "episodes", "successes", "collisions", "reasons")
STATS_SUMS = ("sum_return", "sum_length", "sum_delta_v", "sum_delta_w")


def check_reset_obs(got, want, what="reset obs"):
    np.testing.assert_allclose(to_numpy(got) if hasattr(got, "detach") else got, want, rtol=0, atol=RESET_OBS_TOL, err_msg=what)


def check_outputs(env, ref, o, r, d, t, reward_tol=REWARD_TOL, episode_rows=True):
    """What a step returns, against the oracle's step `ref`.  The episode rows (length, return, terminal observation) are compared
    where an episode finished on this step: a halted env reports done and its rows are not rewritten."""
    np.testing.assert_array_equal(to_numpy(d), ref["done"], err_msg=f"done, step {t}")
    np.testing.assert_array_equal(to_numpy(env.done_reason), ref["done_reason"], err_msg=f"reason, step {t}")
    np.testing.assert_allclose(to_numpy(o), ref["obs"], rtol=0, atol=OBS_TOL, err_msg=f"obs, step {t}")
    np.testing.assert_allclose(to_numpy(r), ref["reward"], rtol=reward_tol, atol=reward_tol, err_msg=f"reward, step {t}")
    if not episode_rows:
        return
    fin = ref["done"].astype(bool)
    new = fin & (ref["episode_length"] > 0)
    if batch_modes(env)[1] == "reset":
        assert (ref["episode_length"][fin] > 0).all(), f"step {t}: a reset-mode env is done without a finished episode"
    np.testing.assert_array_equal(to_numpy(env.episode_length)[new], ref["episode_length"][new], err_msg=f"episode length, step {t}")
    np.testing.assert_allclose(to_numpy(env.episode_return)[new], ref["episode_return"][new], rtol=RETURN_TOL, atol=RETURN_TOL,
                               err_msg=f"episode return, step {t}")
    np.testing.assert_allclose(to_numpy(env.terminal_obs)[new], ref["terminal_obs"][new], rtol=0, atol=OBS_TOL,
                               err_msg=f"terminal obs, step {t}")


def check_diag(env, orc_or_ref, rows, t, from_step_output, errors=True):
    """The evaluator's flags (exact) and error norms on `rows`: the step's diag output against the oracle step's (`orc_or_ref` is that
    step's dict), or rdv_diagnose of the post-step state against the oracle's diagnose() (`orc_or_ref` is the OracleBatch)."""
    if from_step_output:
        got, want = to_numpy(env.diag)[rows], orc_or_ref["diag"][rows]
    else:
        got, want = to_numpy(env.diagnose())[rows], orc_or_ref.diagnose()[rows]
    np.testing.assert_array_equal(got[:, DIAG_FLAGS], want[:, DIAG_FLAGS], err_msg=f"flags, step {t}")
    if errors:
        np.testing.assert_allclose(got[:, DIAG_ERRORS], want[:, DIAG_ERRORS], rtol=DIAG_TOL, atol=DIAG_TOL, err_msg=f"errors, step {t}")


def check_state(env, orc, storage, t, aux=True):
    tol = STATE_TOL[storage]
    np.testing.assert_allclose(to_numpy(env.get_state()), orc.get_state(), rtol=tol, atol=tol, err_msg=f"state, step {t}")
    if aux:
        a_gpu, a_ref = to_numpy(env.get_aux()), orc.get_aux()
        np.testing.assert_array_equal(a_gpu[:, AUX_EXACT], a_ref[:, AUX_EXACT], err_msg=f"t/collided/success/episode, step {t}")
        np.testing.assert_allclose(a_gpu[:, AUX_REAL], a_ref[:, AUX_REAL], rtol=AUX_TOL, atol=AUX_TOL, err_msg=f"aux reals, step {t}")


def check_stats(env, orc, sums=True):
    sg, so = env.get_stats(), orc.get_stats()
    for k in STATS_COUNTERS:
        assert sg[k] == so[k], (k, sg[k], so[k])
    for k in STATS_SUMS if sums else ():
        assert abs(sg[k] - so[k]) <= STATS_SUM_TOL * max(1.0, abs(so[k])), (k, sg[k], so[k])


def live_rows(env, ref):
    """The rows whose post-step state is the one the step produced: not the done rows in reset mode (they hold the next episode)."""
    return ~ref["done"].astype(bool) if batch_modes(env)[1] == "reset" else np.ones(env.num_envs, bool)


def run_against_oracle(env, orc, actions, storage, variant, *, evaluator=False, tape=False, reward_tol=REWARD_TOL, episode_rows=True,
                       diag_every=1, diag_errors=True, state_every=1, aux=True, stats_sums=True, on_step=None):
    """Step `env` (on the device the actions go to: env.device) and `orc` through the float32 [N, 6] arrays `actions`.
    Training path (evaluator=False): steps without diag, so the variant's own kernel runs (asserted each step unless variant is None);
    the evaluator's flags and error norms come from rdv_diagnose of the post-step state, on live_rows().
    Evaluator path: steps with diag, the evaluator build (asserted each step), its diag outputs against the oracle's, every row.
    on_step(orc, ref, t) runs after each step's checks; the statistics are compared at the end."""
    import torch
    for t, a in enumerate(actions):
        o, r, d = env.step(torch.from_numpy(a).to(env.device), diag=evaluator)
        if variant is not None:
            expect_kernel(env, variant, diag=evaluator, tape=tape, what=f"step {t}")
        ref = orc.step(a, want_diag=evaluator)
        check_outputs(env, ref, o, r, d, t, reward_tol=reward_tol, episode_rows=episode_rows)
        if t % diag_every == 0:
            if evaluator:
                check_diag(env, ref, slice(None), t, True, errors=diag_errors)
            else:
                check_diag(env, orc, live_rows(env, ref), t, False, errors=diag_errors)
        if t % state_every == 0:
            check_state(env, orc, storage, t, aux=aux)
        if on_step is not None:
            on_step(orc, ref, t)
    check_stats(env, orc, sums=stats_sums)


def replay_golden(env, g, *, halt, diag, variant=None, obs_tol, reward_kw, reward_dtype=np.float32, bookkeeping=True):
    """The reference's own recorded transitions `g` (tests/golden/steps_*.npz) through `env` (fp64 storage): with its reset tape in
    reset mode, from set_state in halt mode.  `obs_tol`, `reward_kw` and the dtype the recorded fp64 reward is compared in are the call
    site's; diag errors 1e-9 and state / aux 1e-10 absolute (fp64 storage against fp64 records).  bookkeeping adds the initial state,
    aux and diag records, the aux record of every step and the reason flag bits (entered the KOZ, had a success step)."""
    import torch
    T = g["actions"].shape[0]
    if not halt:
        env.set_reset_tape(torch.from_numpy(np.nan_to_num(g["tape"])))
    obs = to_numpy(env.reset())
    if halt:
        env.set_state(torch.from_numpy(g["state0"]))
        obs = to_numpy(env.observe())
    np.testing.assert_array_equal(obs, g["obs0"])
    if bookkeeping:
        np.testing.assert_allclose(to_numpy(env.get_state()), g["state0"], rtol=0, atol=1e-15)
        np.testing.assert_allclose(to_numpy(env.get_aux())[:, :6], g["aux0"], rtol=0, atol=1e-15)
        np.testing.assert_allclose(to_numpy(env.diagnose()), g["diag0"], rtol=0, atol=1e-12)
    n_done = 0
    for t in range(T):
        v = g["valid"][t].astype(bool)
        if not v.any():
            break
        o, r, d = env.step(torch.from_numpy(g["actions"][t]).to(env.device), diag=diag)
        if variant is not None:
            expect_kernel(env, variant, diag=diag, tape=not halt, after_set_state=halt and t == 0, what=f"step {t}")
        o, r, d = to_numpy(o), to_numpy(r), to_numpy(d).astype(bool)
        gd = g["done"][t].astype(bool)
        np.testing.assert_array_equal(d[v], gd[v], err_msg=f"done, step {t}")
        np.testing.assert_array_equal(to_numpy(env.done_reason)[v] & 7, g["reason"][t][v], err_msg=f"reason, step {t}")
        np.testing.assert_allclose(r[v], g["reward"][t][v].astype(reward_dtype), err_msg=f"reward, step {t}", **reward_kw)
        np.testing.assert_allclose(o[v], g["obs_ret"][t][v], rtol=0, atol=obs_tol, err_msg=f"obs, step {t}")
        keep = v if halt else (v & ~gd)          # after an auto-reset the terminal state is gone
        fin = v & gd
        if diag:
            dg, rows = to_numpy(env.diag), v
        else:                                    # the same numbers from the state as it stands (not done rows in reset mode)
            dg, rows = to_numpy(env.diagnose()), keep
        np.testing.assert_array_equal(dg[rows][:, DIAG_FLAGS], g["diag"][t][rows][:, DIAG_FLAGS], err_msg=f"flags, step {t}")
        np.testing.assert_allclose(dg[rows][:, DIAG_ERRORS], g["diag"][t][rows][:, DIAG_ERRORS], rtol=0, atol=1e-9)
        np.testing.assert_allclose(to_numpy(env.get_state())[keep], g["state"][t][keep], rtol=0, atol=1e-10, err_msg=f"state, step {t}")
        np.testing.assert_allclose(to_numpy(env.terminal_obs)[fin], g["obs_step"][t][fin], rtol=0, atol=obs_tol)
        if bookkeeping:
            # bit 4: the episode entered the KOZ (the latched flag), bit 5: it had a success step (the count of the terminal state)
            flags = (g["diag"][t][:, 7] != 0) * 16 + (g["aux"][t][:, 3] > 0) * 32
            np.testing.assert_array_equal(to_numpy(env.done_reason)[fin] & 48, flags[fin], err_msg=f"reason flags, step {t}")
            np.testing.assert_allclose(to_numpy(env.get_aux())[keep][:, :6], g["aux"][t][keep], rtol=0, atol=1e-10)
        n_done += int(fin.sum())
    st = env.get_stats()
    assert st["episodes"] == n_done == int(g["done"].sum())
    assert st["reasons"] == [int((g["reason"] == k).sum()) for k in (1, 2, 3, 4)]

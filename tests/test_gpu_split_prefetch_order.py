"""
GPU tests (run with `-m gpu`) of the order in which the slot form of step_kernel_split (csrc/rdv_step.h) issues its service waves'
requests: chunk 5 and the tag first, the twelve record requests behind their arrival.  Only when a load is issued changed, so the
slot form must still give the bits of the speculative form and both must equal the oracle (tests/parity.py), here at the batch sizes
tests/test_gpu_split_slots.py does not reach and where the service waves' clamped lanes carry most of the requests:

  N = 1    every lane of every service wave reads env 0's chunk 5, tag and record; three service waves have no env at all;
  N = 65   a one-lane second wave;
  N = 256  exactly one full step workgroup and one refill workgroup.
"""
import numpy as np
import pytest

import parity
from helpers import counter_actions, expect_kernel
from oracle_engine import OracleModel
from reinforcement_learning_rendezvous_amd.params import make_params
from test_gpu_split_slots import _both_forms, _finish, _same_bits, _states_agree, _step_all

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = (1, 65, 256)
T = 60
SEED = 17
# t_max = 7 with the default reset ranges: every episode runs its 7 steps (the oracle, 65,536 episodes under counter_actions: no other
# length), so no seed gives a first-step end.  The mix widens the chaser's initial attitude range beyond max_attitude_error (30 deg): ~12 %
# of the episodes then end on their first step, a few on steps 2-6, the rest at the time limit.  Seeds found with the oracle on the CPU
# (episode lengths 1 / 6 / 7 x 7 at N = 1 within T steps).
MIX = dict(t_max=7.0, qc0_range=float(np.radians(40.0)))
MIX_SEED = {1: 18, 65: 17, 256: 17}


def _start(monkeypatch, n, p, seed):
    envs = _both_forms(monkeypatch, n, p, seed=seed)
    orc = OracleModel(n, p, "f32", seed=seed, n_threads=8)
    o0 = orc.reset()
    for env in envs.values():
        parity.check_reset_obs(env.reset(), o0)
    _same_bits(envs["speculative"].obs, envs["slots"].obs, "reset obs")
    return envs, orc


def _run(envs, orc, n, t0, steps, action_seed=5, after_set_state=False):
    """`steps` steps of both forms and the oracle; the oracle's episode lengths at the ends"""
    lengths = []
    for t in range(t0, t0 + steps):
        ref = _step_all(envs, orc, counter_actions(action_seed, t, n), t)
        for env in envs.values():              # (the first step behind rdv_set_state is the raw build of step_kernel)
            expect_kernel(env, "split", after_set_state=after_set_state and t == t0, what=f"step {t}")
        lengths.append(np.asarray(ref["episode_length"])[np.asarray(ref["done"]).astype(bool)])
        if t % 20 == 0:
            _states_agree(envs, orc, t)
    return np.concatenate(lengths)


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_is_the_fallback(monkeypatch, n):
    """t_max = 1: every env ends on the first step of its episode (k == 0 at entry), so no slot can be consumed and no record is used."""
    envs, orc = _start(monkeypatch, n, make_params(t_max=1.0), SEED)
    lengths = _run(envs, orc, n, 0, T)
    assert len(lengths) == n * T and (lengths == 1).all()
    _finish(envs, orc, T)


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_is_a_copy(monkeypatch, n):
    """t_max = 2: every env ends on the second step of its episode, behind the launch that refilled its slot."""
    envs, orc = _start(monkeypatch, n, make_params(t_max=2.0), SEED)
    lengths = _run(envs, orc, n, 0, T)
    assert len(lengths) == n * (T // 2) and (lengths == 2).all()
    _finish(envs, orc, T)


@pytest.mark.parametrize("n", SIZES)
def test_a_mix_of_copies_and_fallbacks(monkeypatch, n):
    """t_max = 7 (MIX, above): ends by attitude error on the first step and later, and by time-out.  By the oracle's own episode lengths
    at least one episode ended on its first step (the fallback) and at least one later (a copy) at this N within the run."""
    envs, orc = _start(monkeypatch, n, make_params(**MIX), MIX_SEED[n])
    lengths = _run(envs, orc, n, 0, T)
    assert (lengths == 1).any(), "no episode ended on its first step"
    assert (lengths > 1).any(), "no episode ended behind its first step"
    _finish(envs, orc, T)


def test_after_reset_mask_and_set_state_the_tags_are_fresh(monkeypatch):
    """N = 65: 20 slot-form steps, reset(mask) on a few envs and set_state on one, 20 more steps.  The calls clear the handle's
    step_slots_ok, the tags are re-derived in front of the next launch, and what a service lane requests follows the fresh tags."""
    n = 65
    envs, orc = _start(monkeypatch, n, make_params(**MIX), MIX_SEED[n])
    _run(envs, orc, n, 0, 20)
    mask = np.zeros(n, dtype=np.uint8)
    mask[[0, 3, 63, 64]] = 1                           # both waves, the one-lane wave's env included
    orc.reset(mask)
    for env in envs.values():
        env.reset(torch.from_numpy(mask).cuda())
    s = orc.get_state()
    s[7, :3] *= 0.5                                     # one chaser at half its distance, mid-episode
    orc.set_state(s)
    for env in envs.values():
        env.set_state(torch.from_numpy(s).cuda())
    lengths = _run(envs, orc, n, 20, 20, after_set_state=True)
    assert len(lengths) > n
    _finish(envs, orc, 40)

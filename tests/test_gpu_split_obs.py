"""
GPU tests (run with `-m gpu`) of the fourth form of step_kernel_split for fp32 storage and on_done = reset (csrc/rdv_step.h):

  speculative       the service waves compute every env's next initial state beside the step waves;
  slots             the service waves prefetch every env's prepared slot and wait;
  slots_target      the slot form whose service waves also run the target's side of the transition (step_kernel_split_target);
  slots_target_obs  the target form whose service waves also form the observation and its Box test, from the chaser half the step wave
                    posts at the join (step_kernel_split_obs): the termination decision is assembled from two waves, and the service
                    wave stores the terminal rows and every observation row.

RDV_SPLIT_FORM, read by rdv_create, picks the form of a handle: the four run in one process.  The new form must give the bits of the three
others on every step — the same functions run on the same inputs, only on another wave — and every form equals the oracle in the sense
of tests/parity.py.  No tolerance beyond parity.py's is involved.  The cases are those of tests/test_gpu_split_target.py at the sizes where
a service wave has no env (1), one lane (65), a whole workgroup (256), a second workgroup with one env (257) and ragged waves (773), plus
the two things only this form has: all four termination reasons in one run, most waves holding Box ends (the service wave's test) beside
ends by time, bubble and attitude (the step wave's), and an env that leaves the Box on the step of its time limit (the reason is 1).
"""
import numpy as np
import pytest

import parity
from helpers import capture, counter_actions, expect_kernel, gpu_batch, oracle_batch, shipped_policy, to_numpy
from oracle_engine import OracleModel
from reinforcement_learning_rendezvous_amd.params import make_params
from test_gpu_lazy_branches import KOZ_PARAMS, Branches
from test_gpu_split_prefetch_order import MIX, MIX_SEED
from test_gpu_split_slots import DONE_ROWS, OUTPUTS, _reset_tape, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NEW = "slots_target_obs"
OLD = ("speculative", "slots", "slots_target")
FORMS = OLD + (NEW,)
SIZES = (1, 65, 256, 257, 773)
T = 60
KERNEL = "step_kernel_split<float, true>"      # what every form reports


def _four_forms(monkeypatch, n, params, seed, **kw):
    envs = {}
    for form in FORMS:
        monkeypatch.setenv("RDV_SPLIT_FORM", form)
        envs[form] = gpu_batch(n, params=params, storage="f32", seed=seed, variant="split", **kw)
    monkeypatch.delenv("RDV_SPLIT_FORM")
    return envs


def _outputs_agree(envs, t):
    new = envs[NEW]
    d = new.done.bool()
    for form in OLD:
        old = envs[form]
        for k in OUTPUTS:
            _same_bits(getattr(new, k), getattr(old, k), f"{k}, step {t}: {NEW} differs from {form}")
        for k in DONE_ROWS:
            _same_bits(getattr(new, k)[d], getattr(old, k)[d], f"{k}, step {t}: {NEW} differs from {form}")


def _states_agree(envs, orc, t):
    for form in OLD:
        _same_bits(envs[NEW].get_state(), envs[form].get_state(), f"state, step {t}: {NEW} differs from {form}")
        _same_bits(envs[NEW].get_aux(), envs[form].get_aux(), f"aux, step {t}: {NEW} differs from {form}")
        assert envs[NEW].get_stats() == envs[form].get_stats(), f"stats, step {t}: {NEW} differs from {form}"
    for env in envs.values():
        parity.check_state(env, orc, "f32", t)


def _step_all(envs, orc, a, t, raw=False, tape=False, **step_kw):
    """one step of the four forms and of the oracle: each form against the oracle, the new form against the three others, the kernel"""
    ref = orc.step(a, want_diag=bool(step_kw.get("diag")))
    act = torch.from_numpy(a).cuda()
    for env in envs.values():
        o, r, d = env.step(act, **step_kw)
        parity.check_outputs(env, ref, o, r, d, t)
        expect_kernel(env, "split", diag=bool(step_kw.get("diag")), tape=tape, after_set_state=raw, what=f"step {t}")
    _outputs_agree(envs, t)
    return ref


def _start(monkeypatch, n, p, seed, tape=None):
    envs = _four_forms(monkeypatch, n, p, seed)
    orc = OracleModel(n, p, "f32", seed=seed, n_threads=8, tape=tape)
    if tape is not None:
        dev_tape = torch.from_numpy(tape).cuda()
        for env in envs.values():
            env.set_reset_tape(dev_tape)
    o0 = orc.reset()
    for env in envs.values():
        parity.check_reset_obs(env.reset(), o0)
    return envs, orc


def _run(envs, orc, n, steps, action_seed=5, tape=False, after_step=None):
    """`steps` steps; returns the oracle's episode lengths at the ends"""
    lengths = []
    for t in range(steps):
        ref = _step_all(envs, orc, counter_actions(action_seed, t, n), t, tape=tape)
        assert envs[NEW].last_kernel == KERNEL
        lengths.append(np.asarray(ref["episode_length"])[np.asarray(ref["done"]).astype(bool)])
        if after_step is not None:
            after_step(ref, t)
        if t % 20 == 0:
            _states_agree(envs, orc, t)
    return np.concatenate(lengths)


def _finish(envs, orc, t):
    _states_agree(envs, orc, t)
    for env in envs.values():
        parity.check_stats(env, orc)
        env.close()


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_is_the_fallback(monkeypatch, n):
    """t_max = 1: every env ends on the first step of its episode (the step wave's time test in every lane), every reset is the in-lane
    fallback, and the service wave stores a terminal row for every env on every step."""
    envs, orc = _start(monkeypatch, n, make_params(t_max=1.0), 17)
    lengths = _run(envs, orc, n, T)
    assert len(lengths) == n * T and (lengths == 1).all()
    _finish(envs, orc, T)


@pytest.mark.parametrize("n", SIZES)
def test_every_reset_is_a_copy(monkeypatch, n):
    """t_max = 2: every reset copies a record, all envs of a workgroup end together, and every other step nobody ends: the service wave
    stores the rows with and without a reset observation in them."""
    envs, orc = _start(monkeypatch, n, make_params(t_max=2.0), 17)
    lengths = _run(envs, orc, n, T)
    assert len(lengths) == n * (T // 2) and (lengths == 2).all()
    _finish(envs, orc, T)


@pytest.mark.parametrize("n", SIZES)
def test_a_mix_of_copies_and_fallbacks(monkeypatch, n):
    """The mix of tests/test_gpu_split_prefetch_order.py (t_max = 7, the chaser's initial attitude range beyond the attitude limit):
    copies and first-step fallbacks in one wave."""
    envs, orc = _start(monkeypatch, n, make_params(**MIX), MIX_SEED.get(n, 17))
    lengths = _run(envs, orc, n, T)
    assert (lengths == 1).any(), "no episode ended on its first step"
    assert (lengths > 1).any(), "no episode ended behind its first step"
    assert len(lengths) > 4 * n
    _finish(envs, orc, T)


def _reasons_of(ref):
    """the oracle's reason (1 Box, 2 time, 3 bubble, 4 attitude) of the envs that ended on this step, and their episode lengths"""
    d = np.asarray(ref["done"]).astype(bool)
    return (np.asarray(ref["done_reason"])[d] & 15), np.asarray(ref["episode_length"])[d]


@pytest.mark.parametrize("n", SIZES)
def test_all_four_reasons_in_one_run(monkeypatch, n):
    """Initial positions up to 40 m and velocities up to 1 m/s off the nominal, attitudes up to 40 degrees: episodes end outside the Box
    (reason 1: the service wave's ballot), at the time limit, outside the bubble and beyond the attitude limit (2, 3, 4: the step wave's)
    — on the CPU oracle 11 / 3 / 5 / 9 ends at N = 1, 894 / 226 / 347 / 650 at N = 65 and 10,991 / 2,628 / 4,226 / 8,215 at N = 773 in 60
    steps, so from N = 65 up nearly every wave holds both kinds in nearly every step.  All four must occur, counted from the oracle."""
    p = make_params(t_max=7.0, rc0_range=40.0, vc0_range=1.0, qc0_range=float(np.radians(40.0)))
    envs, orc = _start(monkeypatch, n, p, 17)
    count = np.zeros(5, dtype=np.int64)

    def after_step(ref, t):
        count[:] += np.bincount(_reasons_of(ref)[0], minlength=5)[:5]

    lengths = _run(envs, orc, n, T, after_step=after_step)
    print(f"N = {n}: ends by reason 1 / 2 / 3 / 4: {count[1:].tolist()}")
    assert count[0] == 0 and (count[1:] > 0).all(), count
    assert count.sum() == len(lengths)
    _finish(envs, orc, T)


@pytest.mark.parametrize("n", SIZES)
def test_outside_the_box_on_the_step_of_the_time_limit(monkeypatch, n):
    """Chaser rates up to 20 deg/s off the nominal: some env leaves the Box on the very step its time runs out — the step wave's ballot
    and the service wave's both hold its lane, and the reason must be 1 (the first true of the reference's list).  The oracle shows one
    such coincidence at N = 256 and 257 and two at N = 773; counted from the oracle, at least one must occur there."""
    p = make_params(t_max=7.0, vc0_range=1.0, wc0_range=float(np.radians(20.0)), qc0_range=float(np.radians(40.0)))
    envs, orc = _start(monkeypatch, n, p, 17)
    k_time = int(round(p.t_max / p.dt))
    count = {"both": 0, "box": 0, "time": 0}

    def after_step(ref, t):
        reason, length = _reasons_of(ref)
        assert (length <= k_time).all()
        count["both"] += int(((reason == 1) & (length == k_time)).sum())
        count["box"] += int((reason == 1).sum())
        count["time"] += int((reason == 2).sum())

    _run(envs, orc, n, T, after_step=after_step)
    print(f"N = {n}: {count}")
    if n >= 256:
        assert count["both"] >= 1, count
        assert count["box"] > count["both"] and count["time"] > 0, count
    _finish(envs, orc, T)


@pytest.mark.parametrize("pname", list(KOZ_PARAMS))
def test_the_lazy_branches_beside_the_service_wave_s_observation(monkeypatch, pname):
    """The run of tests/test_gpu_lazy_branches.py::test_keep_out_zone_parameters_vs_oracle (N = 512, seed 21, 24 steps, actions scaled by
    0.3): chasers inside the keep-out zone and at the docking port, where the finish — here without its observation — takes its lazy
    branches.  Collisions, success steps and bonus steps are counted from the oracle and must all occur."""
    n, steps, seed = 512, 24, 21
    p = make_params(**KOZ_PARAMS[pname])
    envs = _four_forms(monkeypatch, n, p, seed)
    orc = oracle_batch(n, p, "f32", "reset", seed=seed, n_threads=8)
    o0 = orc.reset()
    for env in envs.values():
        parity.check_reset_obs(env.reset(), o0)
        np.testing.assert_array_equal(to_numpy(env.get_aux())[:, [2, 3]], orc.get_aux()[:, [2, 3]])
    br = Branches(p)
    for t in range(steps):
        ref = _step_all(envs, orc, (counter_actions(seed + 40, t, n) * 0.3).astype(np.float32), t)
        rows = parity.live_rows(envs[NEW], ref)
        for env in envs.values():
            parity.check_diag(env, orc, rows, t, False)
        _states_agree(envs, orc, t)
        br.add(orc, ref, rows)
    br.check(f"{pname} {NEW}")
    _finish(envs, orc, steps)


def test_the_reset_tape(monkeypatch):
    """t_max = 5 with a reset tape of depth 3 (tests/test_gpu_split_slots.py), N = 257: the refill workgroups and the fallback read
    their tape rows."""
    n = 257
    p = make_params(t_max=5.0)
    envs, orc = _start(monkeypatch, n, p, 17, tape=_reset_tape(n, p))
    lengths = _run(envs, orc, n, T, tape=True)
    assert len(lengths) > 4 * n
    _finish(envs, orc, T)


def test_a_step_after_whatever_invalidates_the_slots(monkeypatch):
    """The sequence of test_gpu_split_slots.py::test_a_slot_form_step_after_whatever_invalidates_the_slots with the new form beside the
    three others: a step right behind set_params, seed + reset, reset(mask), set_state (the next step is the raw build), restore, a diag
    step, rdv_step_many and rdv_rollout."""
    n = 773
    p = make_params(t_max=4.0)
    envs = _four_forms(monkeypatch, n, p, seed=9)
    orc = OracleModel(n, p, "f32", seed=9, n_threads=8)
    pols = {f: shipped_policy("cuda:0", noise_seed=4) for f in FORMS}
    step = [0]
    n_done = [0]

    def run(k, raw=False, **step_kw):
        for j in range(k):
            ref = _step_all(envs, orc, counter_actions(6, step[0], n), step[0], raw=raw and j == 0, **step_kw)
            n_done[0] += int(ref["done"].sum())
            step[0] += 1

    def everyone(f):
        for e in list(envs.values()) + [orc]:
            f(e)

    def reset_all():
        o0 = orc.reset()
        for env in envs.values():
            parity.check_reset_obs(env.reset(), o0)

    reset_all()
    run(9)
    q = make_params(t_max=3.0, rc0_range=2.0, qt0_range=float(np.radians(10.0)))
    everyone(lambda e: e.set_params(q))
    run(9)
    everyone(lambda e: e.seed(41))
    reset_all()
    run(7)
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    orc.reset(mask)
    for env in envs.values():
        env.reset(torch.from_numpy(mask).cuda())
    run(7)
    s = orc.get_state()
    s[:, :3] *= 0.5                                     # every chaser at half its distance, mid-episode
    orc.set_state(s)
    for env in envs.values():
        env.set_state(torch.from_numpy(s).cuda())
    run(8, raw=True)
    snaps = {f: e.snapshot() for f, e in envs.items()}
    snap_o = orc.snapshot()
    run(6)
    for f, e in envs.items():
        e.restore(snaps[f])
    orc.restore(snap_o)
    run(8, raw=True)
    run(2, diag=True)
    run(8)
    K = 6
    tape = np.stack([counter_actions(6, step[0] + j, n) for j in range(K)])
    outs = {f: e.step_many(torch.from_numpy(tape).cuda()) for f, e in envs.items()}
    for j in range(K):
        ref = orc.step(tape[j])
        for f in FORMS:
            np.testing.assert_array_equal(to_numpy(outs[f]["done"][j]), ref["done"], err_msg=f"step_many done, row {j}")
            np.testing.assert_allclose(to_numpy(outs[f]["obs"][j]), ref["obs"], rtol=0, atol=parity.OBS_TOL, err_msg=f"step_many obs, row {j}")
    step[0] += K
    run(8)
    ros = {f: e.rollout(pols[f], K) for f, e in envs.items()}
    for f in OLD:
        _same_bits(ros[NEW]["actions"], ros[f]["actions"], "rollout actions")
    acts = to_numpy(torch.clamp(ros[NEW]["actions"], -1.0, 1.0))
    for j in range(K):
        ref = orc.step(acts[j])
        for f in FORMS:
            np.testing.assert_array_equal(to_numpy(ros[f]["done"][j]), ref["done"], err_msg=f"rollout done, row {j}")
    run(8)
    assert envs[NEW].last_kernel == KERNEL
    assert n_done[0] > 4 * n
    for pol in pols.values():
        pol.close()
    _finish(envs, orc, step[0])


def test_graph_replay_of_the_new_form_equals_eager_steps(monkeypatch):
    """16 steps recorded once and replayed three times against the same steps made eagerly, every output buffer of every step, bit for
    bit (tests/test_gpu_split_slots.py, tests/test_gpu_graphs.py)."""
    n, K, replays = 773, 16, 3
    p = make_params(t_max=6.0)
    monkeypatch.setenv("RDV_SPLIT_FORM", NEW)
    graphed, eager = (gpu_batch(n, params=p, storage="f32", seed=12, variant="split") for _ in range(2))
    monkeypatch.delenv("RDV_SPLIT_FORM")
    tape = torch.from_numpy(np.stack([counter_actions(7, t, n) for t in range(K)])).cuda()
    names = OUTPUTS + DONE_ROWS

    def steps(env):
        rows = []
        for k in range(K):
            env.step(tape[k])
            rows.append({name: getattr(env, name).clone() for name in names})
        return rows

    for env in (graphed, eager):
        env.reset()
    rec = {}
    g = capture(lambda: rec.update(out=steps(graphed)))
    steps(eager)
    for r in range(replays):
        g.replay()
        want = steps(eager)
        torch.cuda.synchronize()
        for k in range(K):
            for name in names:
                _same_bits(rec["out"][k][name], want[k][name], f"replay {r}, step {k}: {name} differs from the eager calls")
    _same_bits(graphed.get_state(), eager.get_state(), "final state")
    _same_bits(graphed.get_aux(), eager.get_aux(), "final bookkeeping")
    st = graphed.get_stats()
    assert st == eager.get_stats() and st["episodes"] > 4 * n
    assert graphed.last_kernel == eager.last_kernel == KERNEL
    graphed.close(); eager.close()

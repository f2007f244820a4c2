"""
The evaluator's references, on the CPU (no GPU): tests/golden/eval_reference_variants.npz — the reference's own
CustomWandbCallback.evaluate_policy and monte_carlo.evaluate under the configurations sensitivity_analysis.py varies
(tests/golden/make_golden_eval_variants.py) — against the oracle engine and its NumPy restatement of the evaluation accumulators
(tests/oracle_engine.py), which is what tests/test_gpu_evaluator.py holds the kernels to.  Three things:

  1. the restatement reproduces the reference's recorded numbers when it replays the recorded actions (no policy, so no GEMM noise);
  2. its group summaries recombine to the whole-batch summary, and the rows the fp32 GPU comparison drops stay under 5 % per config;
  3. every comparison of tests/evaluator_checks.py can fail: seven defects, each applied to the restatement or to a copy of its
     accumulators, each rejected on the fixture data.

    python tests/test_evaluator_reference.py      # rewrites profiles/evaluator_parity.txt (the measured oracle-vs-reference deviations)
"""
import functools
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script; pytest's conftest does the same)

import numpy as np
import pytest

import evaluator_checks as ec
from helpers import to_numpy
from oracle_engine import OracleEngine
from reinforcement_learning_rendezvous_amd import monte_carlo as mc
from reinforcement_learning_rendezvous_amd.evaluation import SUMMARY_KEYS
from reinforcement_learning_rendezvous_amd.params import make_params

torch = pytest.importorskip("torch")

CASES = ec.fixture_cases()
IDS = [ec.case_id(c) for c in CASES]
DEG = 180.0 / math.pi
STATE_PER_STEP, REWARD_PER_STEP = 8e-14, 5e-13        # the oracle's distance from the reference, per step

# The largest |oracle - fixture| / max(1, |fixture|) per quantity over the configurations, as profiles/evaluator_parity.txt lists them per
# configuration (measured with the recorded actions replayed, fp64 storage).  The assertion is 4 x this, and never tighter than the
# per-step distance above times the configuration's step count.
MEASURED = {
    "cb": {"ep_rew": 4.166e-16, "ep_dist": 1.107e-15, "ep_delta_v": 0.0, "ep_delta_w": 0.0, "ep_min_pos_error": 3.331e-16,
           "ep_avg_att_error": 1.388e-17},
    "mc": {"total_reward": 1.325e-14, "total_delta_v": 0.0, "min_dist_from_koz": 5.551e-15, "pos_error": 3.120e-14, "vel_error": 6.051e-15,
           "att_error": 3.731e-16, "rot_error": 5.551e-15},
}          # every one of them lies below its floor (1e-12 and up): the floors are what the test asserts today


@functools.lru_cache(maxsize=None)
def oracle_run(i, storage="f64"):
    """(engine, history) of fixture case i replayed through the oracle engine; shared by the tests below, which leave both unchanged."""
    c = CASES[i]
    eng = OracleEngine(len(c.state0), c.params, storage=storage, on_done="halt")
    return eng, ec.replay_with_history(eng, c)


def strictest_level(acc):
    hit = np.asarray(acc)[:, ec.LEVEL_COUNT_COLS] > 0
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def deviations(i):
    """{quantity: (largest |oracle - fixture| / max(1, |fixture|), floor)} of the real-valued quantities of case i."""
    c = CASES[i]
    eng, _ = oracle_run(i)
    steps = c.actions.shape[0]
    if c.kind == "cb":
        got, want = eng.eval_summary(), dict(zip(SUMMARY_KEYS, c.reference))
        return {k: (abs(got[k] - want[k]) / max(1.0, abs(want[k])), (REWARD_PER_STEP if k == "ep_rew" else STATE_PER_STEP) * steps)
                for k in ec.REAL_METRICS}
    cols = mc.columns_from_accumulators(eng.eval, eng.get_aux(), c.params)
    out = {}
    for k in ec.REAL_COLUMNS:
        want = c.reference[:, mc.COLUMNS.index(k)]
        floor = (REWARD_PER_STEP if k == "total_reward" else STATE_PER_STEP) * steps * (DEG if k in ("att_error", "rot_error") else 1.0)
        out[k] = (float(np.max(np.abs(cols[k] - want) / np.maximum(1.0, np.abs(want)))), floor)
    return out


# ------------------------------------------------------------------------------------------------ 1. the oracle against the fixture
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_reproduces_the_reference_evaluators(i):
    """The recorded actions replayed through the oracle engine (fp64 storage): the count-derived means at rel 1e-12, the integer Monte
    Carlo columns and the strictest level exactly, every real-valued mean and column within 4 x its measured deviation."""
    c = CASES[i]
    eng, hist = oracle_run(i)
    acc = to_numpy(eng.eval)
    np.testing.assert_array_equal(acc[:, 1], hist.valid[1:].sum(axis=0), err_msg="an episode's length is not the reference's")
    if c.kind == "cb":
        got, want = eng.eval_summary(), dict(zip(SUMMARY_KEYS, c.reference))
        for k in ec.COUNT_METRICS:
            assert got[k] == pytest.approx(want[k], rel=1e-12), k
    else:
        cols = mc.columns_from_accumulators(eng.eval, eng.get_aux(), c.params)
        for k in ec.INT_COLUMNS:
            np.testing.assert_array_equal(cols[k], c.reference[:, mc.COLUMNS.index(k)], err_msg=k)
        np.testing.assert_array_equal(strictest_level(acc), c.level, err_msg="strictest level reached")
    for k, (dev, floor) in deviations(i).items():
        print(f"{ec.case_id(c)} {k}: {dev:.3e} (bound {max(4 * MEASURED[c.kind][k], floor):.3e})")
        assert dev <= max(4 * MEASURED[c.kind][k], floor), (k, dev, MEASURED[c.kind][k], floor)


def test_fixture_shows_every_branch_of_the_evaluators():
    """What make_golden_eval_variants.py asserted when it wrote the file, read back from the committed file."""
    cb = {c.name: dict(zip(SUMMARY_KEYS, c.reference)) for c in CASES if c.kind == "cb"}
    assert {round(float(c.params.dt), 3) for c in CASES} >= {0.5, 0.1}
    assert all(c.actions.shape[0] <= 60 and len(c.state0) % 4 != 0 for c in CASES if c.kind == "cb")
    assert any(m["ep_time_of_first_collision"] == -1 and m["%_collided_episodes"] == 0 for m in cb.values())
    assert any(m["%_collided_episodes"] == 100 for m in cb.values())
    assert any(m["ep_min_pos_error"] == -1 and m["ep_time_of_first_collision"] == 0 for m in cb.values())
    assert any(0 < m["%_collided_episodes"] < 100 for m in cb.values())
    levels = np.concatenate([c.level for c in CASES if c.kind == "mc"])
    assert set(levels.astype(int).tolist()) == {-1, 0, 1, 2, 3}
    assert all(len(c.state0) == 32 for c in CASES if c.kind == "mc")


# ------------------------------------------------------------------------------------------------ 2. dropped rows, groups
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_rows_near_a_decision_stay_under_five_percent(i):
    """The fp32 GPU comparison drops the rows whose fp64 oracle trajectory comes within parity.DIAG_TOL of a decision
    (evaluator_checks.near_decision); from the oracle alone: at most 5 % of a configuration's rows.  The cosines that rule reads off
    the state are the oracle's own: its attitude error and its collision flag follow from them at every sample."""
    c = CASES[i]
    _, hist = oracle_run(i)
    near = ec.near_decision(c.params, hist)
    print(f"{ec.case_id(c)}: {int(near.sum())} of {len(near)} rows near a decision")
    assert near.mean() <= 0.05
    x_att, x_cor, r = ec.grid_cosines(c.params, hist.state)
    v = hist.valid
    np.testing.assert_allclose(np.arccos(np.rint(x_att[v]) / 1e5), hist.diag[..., 2][v], rtol=0, atol=1e-12)
    koz = (r < c.params.koz_radius) & (np.arccos(np.clip(np.rint(x_cor) / 1e5, -1, 1)) > c.params.corridor_half_angle)
    far = np.abs(x_cor - np.rint(x_cor)) < 0.49                     # (not within 1e-7 of a rounding tie of the grid itself)
    np.testing.assert_array_equal(koz[v & far], hist.diag[..., 4][v & far] != 0)


@functools.lru_cache(maxsize=None)
def grouped_run():
    return ec.grouped_oracle("f64")[0]


def test_grouped_batch_rows_near_a_decision_stay_under_five_percent():
    """The fp32 group test of tests/test_gpu_evaluator.py drops rows by the same rule, each group under its own parameters."""
    _, hist = ec.grouped_oracle("f64")
    keep = ec.grouped_keep(hist)
    starts = np.concatenate([[0], np.cumsum(ec.GROUP_SIZES)])
    shares = [1.0 - keep[a:b].mean() for a, b in zip(starts[:-1], starts[1:])]
    print("dropped share per group:", shares)
    assert max(shares) <= 0.05


def test_group_summaries_recombine_to_the_whole_batch():
    """eval_summary(rows=) of the restatement on a grouped batch (each group's own dt): the mean-type entries of the three groups,
    weighted by their episode counts, are the whole batch's; each group summary is the fsum reference of its rows within the reduction's
    bound; and the batch shows collided and collision-free episodes in every group."""
    eng = grouped_run()
    sizes, n = ec.GROUP_SIZES, sum(ec.GROUP_SIZES)
    whole = eng.eval_summary()
    parts = [eng.eval_summary(group=g) for g in range(len(sizes))]
    for k in ec.MEAN_METRICS:
        assert sum(m * s[k] for m, s in zip(sizes, parts)) / n == pytest.approx(whole[k], rel=1e-12), k
    acc, aux, st = to_numpy(eng.eval), to_numpy(eng.get_aux()), to_numpy(eng.get_state())
    dt = eng._orc.row_params("dt")
    assert sorted(set(dt.tolist())) == [0.25, 0.5, 1.0]
    ec.check_reduction(whole, acc, aux, st, dt, "whole batch")
    for g, s in enumerate(parts):
        rows = eng._orc.group_rows(g)
        ec.check_reduction(s, acc[rows], aux[rows], st[rows], dt[rows], f"group {g}")
        assert 0 < s["%_collided_episodes"] < 100, (g, s)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match=f"group {bad} of 3"):
            eng.eval_summary(group=bad)


# ------------------------------------------------------------------------------------------------ 3. every comparison can fail
def _rejected(check, *a, **k):
    try:
        check(*a, **k)
    except AssertionError:
        return True
    return False


def _att_sum_without_k0(acc, hist, eng):
    out = acc.copy()
    out[:, 2] -= hist.diag[0, :, 2]
    return out


def _first_collision_one_step_late(acc, hist, eng):
    out = acc.copy()
    out[:, 4] += eng.params.dt                                        # (NaN stays NaN)
    return out


def _min_pos_updated_after_the_first_collision(acc, hist, eng):
    free = hist.valid & (hist.diag[..., 4] == 0)
    lowest = np.where(free, hist.diag[..., 0], np.inf).min(axis=0)
    out = acc.copy()
    rows = ~np.isnan(acc[:, 5])
    out[rows, 5] = np.minimum(acc[rows, 5], lowest[rows])
    return out


def _level_sum_started_one_step_late(acc, hist, eng):
    out = acc.copy()
    hits = np.stack([np.stack(eng._orc._levels(d), axis=1) for d in hist.diag]) & hist.valid[..., None]      # [T+1, N, 4]
    for L in range(4):
        rows = np.flatnonzero(hits[..., L].any(axis=0))
        first = hits[..., L].argmax(axis=0)[rows]
        out[rows, 12 + 5 * L] -= 1
        out[rows, 13 + 5 * L: 17 + 5 * L] -= hist.diag[first, rows, 0:4]
    return out


ACCUMULATOR_DEFECTS = {"the k = 0 sample dropped from the attitude sum": _att_sum_without_k0,
                       "the time of first collision taken one step late": _first_collision_one_step_late,
                       "column 5 updated after the first collision": _min_pos_updated_after_the_first_collision,
                       "a level's sum started one step after its first hit": _level_sum_started_one_step_late}


@pytest.mark.parametrize("defect", list(ACCUMULATOR_DEFECTS))
def test_accumulator_defects_are_rejected(defect):
    """Each defect applied to a copy of the restatement's accumulators, per fixture configuration: wherever it changes anything, the
    fp64 accumulator comparison of tests/test_gpu_evaluator.py rejects the copy — and it changes something in at least two configurations."""
    changed = 0
    for i, c in enumerate(CASES):
        eng, hist = oracle_run(i)
        good = to_numpy(eng.eval)
        bad = ACCUMULATOR_DEFECTS[defect](good, hist, eng)
        ec.check_accumulators(good.copy(), good, "f64")
        if not np.array_equal(bad, good, equal_nan=True):
            changed += 1
            assert _rejected(ec.check_accumulators, bad, good, "f64"), (defect, ec.case_id(c))
    assert changed >= 2, (defect, changed)


def test_steps_for_steps_plus_one_is_rejected():
    """ep_avg_att_error formed with `steps` for `steps + 1` (custom_callbacks.py:268): rejected by the summary comparison and by the
    reduction's fsum reference, in every configuration."""
    for i, c in enumerate(CASES):
        eng, _ = oracle_run(i)
        acc, aux, st = to_numpy(eng.eval), to_numpy(eng.get_aux()), to_numpy(eng.get_state())
        good = eng.eval_summary()
        bad = dict(good, ep_avg_att_error=float((acc[:, 2] / (aux[:, 0] / c.params.dt)).mean()))
        ec.check_summary(dict(good), good)
        ec.check_reduction(good, acc, aux, st, c.params.dt)
        assert _rejected(ec.check_summary, bad, good), ec.case_id(c)
        assert _rejected(ec.check_reduction, bad, acc, aux, st, c.params.dt), ec.case_id(c)


def test_a_group_summary_over_one_wave_too_many_is_rejected():
    """The restatement summing [first, last + 64) for a group: rejected by the fsum reference over the group's rows, for both groups
    that have a successor."""
    eng = grouped_run()
    acc, aux, st = to_numpy(eng.eval), to_numpy(eng.get_aux()), to_numpy(eng.get_state())
    dt = eng._orc.row_params("dt")
    for g in (0, 1):
        rows = eng._orc.group_rows(g)
        bad = eng._orc.eval_summary(rows=slice(rows.start, rows.stop + 64))
        assert _rejected(ec.check_reduction, bad, acc[rows], aux[rows], st[rows], dt[rows]), g


def _limit_rows_on_the_oracle(levels=None):
    """eval_begin, and one zero-action accumulate step for the fixed-point rows, of the threshold rows on the oracle engine; `levels`
    replaces the restatement's level decisions.  -> [(section, p, rows, acc0, fixed mask, acc1 of the fixed rows)]"""
    from helpers import load_golden
    g = load_golden("thresholds_reference.npz")
    out = []
    for section, p, rows in ec.limit_rows():
        eng = OracleEngine(len(rows), make_params(), storage="f64", on_done="halt")
        if levels is not None:
            eng._orc._levels = types.MethodType(levels, eng._orc)
        eng.reset()                                                   # under the default parameters: no flag latches
        eng.set_params(p)
        eng.set_state(torch.from_numpy(g[f"{section}_state"][rows]))
        acc0 = to_numpy(eng.eval_begin()).copy()
        eng.step(torch.zeros((len(rows), 6)), accumulate=True)
        fixed = g[f"{section}_fixed"][rows] == 1
        out.append((section, p, rows, acc0, fixed, to_numpy(eng.eval)[fixed]))
    return out


def _check_limit_rows(results):
    for section, p, rows, acc0, fixed, acc1 in results:
        ec.check_level_counts(acc0, ec.expected_level_counts(section, p, rows, False), f"{section} eval_begin")
        ec.check_level_counts(acc1, ec.expected_level_counts(section, p, rows[fixed], True), f"{section} after one step")


def test_level_counts_on_their_limits_and_a_non_strict_comparison_is_rejected():
    """States on a constraint limit and 1-2 ulp either side (thresholds_reference.npz): the restatement's level counts are what strict `<`
    gives on the reference's own recorded errors; `<=` in any ONE of the four comparisons is rejected."""
    _check_limit_rows(_limit_rows_on_the_oracle())
    for j in range(4):
        def levels(self, d, j=j):
            lim = [self.row_params(f) for f in ec.LIMIT_FIELDS]
            m = [(d[:, k] <= lim[k]) if k == j else (d[:, k] < lim[k]) for k in range(4)]
            return [m[0] & m[1] & m[2] & m[3], (m[0] & m[1] & m[2]) | (m[0] & m[1] & m[3]), m[0] & m[1], m[0]]
        assert _rejected(_check_limit_rows, _limit_rows_on_the_oracle(levels)), ec.LIMIT_FIELDS[j]


# ------------------------------------------------------------------------------------------------ the profile
def write_profile(path):
    lines = ["# |oracle - fixture| / max(1, |fixture|) of every real-valued quantity of tests/golden/eval_reference_variants.npz, the recorded",
             "# actions replayed through the oracle engine in fp64 storage (tests/test_evaluator_reference.py; att_error / rot_error in degrees).",
             "# config quantity deviation floor(steps x per-step distance of DESIGN.md §3)"]
    worst = {"cb": {}, "mc": {}}
    for i, c in enumerate(CASES):
        for k, (dev, floor) in deviations(i).items():
            lines.append(f"{ec.case_id(c)} {k} {dev:.3e} {floor:.3e}")
            worst[c.kind][k] = max(worst[c.kind].get(k, 0.0), dev)
    lines.append("# largest per quantity (MEASURED in the test):")
    lines += [f"# {kind} {k} {v:.3e}" for kind in worst for k, v in worst[kind].items()]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return worst


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(write_profile(os.path.join(root, "profiles", "evaluator_parity.txt")))

"""
GPU tests (run with `-m gpu`): the seeded call sequences of tests/call_sequences.py on a RendezvousBatch.

Subject: a RendezvousBatch driven exactly as the program says (rdv_step in every variant, rdv_step_many, rdv_rollout, act + step, the
evaluator build), so its host flags and slot tags go through whatever the program's changers do to them.
Model: tests/oracle_engine.py::OracleModel, which has no such state; tests/parity.py's checks with its constants after every consumer,
observe / state / aux after every changer, the statistics with their sums at the end and at every stats_reset.
Twin: a second RendezvousBatch with the same constructor arguments and variant="fused_inlane" that receives every changer (but the
variant switches) and performs every consumer as plain rdv_step calls with a policy object of its own: it never launches a persistent
kernel and never holds a slot.  Everything is compared with it bit for bit, get_stats() dicts included — what the oracle's tolerances
cannot see.
After every consumer the subject's last_kernel is checked against the dispatch rules (call_sequences.State.kernel);
tests/test_call_sequences.py shows from the generator and the same rules that every dispatchable name is expected somewhere.

RDV_SEQ=profile:seed[:upto] runs one program, cut after ``upto`` ops.
"""
import os
import time

import pytest

import call_sequences as cs
from helpers import gpu_batch, shipped_policy
from oracle_engine import OracleModel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SELECTED = os.environ.get("RDV_SEQ")
PROGRAMS = [cs.parse_selection(SELECTED)[:2]] if SELECTED else cs.all_programs()
UPTO = cs.parse_selection(SELECTED)[2] if SELECTED else None


def _run(ops, profile, seed, upto=None):
    n, params, kw = cs.engine_kwargs(profile, seed)
    subject, twin = gpu_batch(n, params=params, **kw), gpu_batch(n, params=params, variant="fused_inlane", **kw)
    policies = [shipped_policy("cuda:0", noise_seed=seed) for _ in range(2)]
    r = None
    t0 = time.perf_counter()
    try:
        r = cs.run(ops, subject, OracleModel(n, params, **kw), twin=twin, upto=upto, profile=profile, seed=seed, policy=policies[0],
                   twin_policy=policies[1])
    finally:
        for e in ([r.subject, r.twin] if r is not None else []) + policies:
            e.close()
    print(f"{profile}:{seed}: {len(ops)} ops, {time.perf_counter() - t0:.2f} s")
    return r


@pytest.mark.parametrize("profile,seed", PROGRAMS, ids=[f"{p}:{s}" for p, s in PROGRAMS])
def test_program_agrees_with_the_oracle_and_the_plain_step_twin(profile, seed):
    ops = cs.program(profile, seed)
    r = _run(ops, profile, seed, upto=UPTO)
    if UPTO is None:                       # one name per consumer: every consumer's kernel was checked
        assert len(r.kernels) == sum(op[0] in cs.CONSUMERS for op in ops)


# Regression programs: the shortest forms of what the seeded programs found (the seeded programs that found them stay in SEEDS).
REGRESSIONS = {
    # clone() of a grouped batch created the copy from group 0's parameters, so that ungrouping the copy returned to group 0's set
    # instead of the set the original was given last (groups:30, op 19: observations of every env on another position scale,
    # -0.752 against -0.474)
    "ungrouping-a-clone": ("groups", 30, [("group_on", 2, (3, 1, 0)), ("reset_full",), ("step",), ("clone",), ("group_off",), ("step_many", 2)]),
    # rdv_step_many / rdv_rollout summed a launch's statistics on their own and added the total to the wave's slot: slot + (s1 + s2)
    # where the rdv_step loop computes (slot + s1) + s2 — with fp64 storage the last bit of sum_return / sum_delta_w (reset-f64:29:
    # 46185.849302658135 against 46185.84930265814).  Parameter set 1 ends every episode at every step.
    "statistics-order-f64": ("reset-f64", 29, [("reset_full",), ("set_params", 1), ("step_many", 9), ("step",), ("rollout", 5, False),
                                               ("step_many", 5), ("stats_reset",), ("rollout", 9, True), ("step_many", 2)]),
}


@pytest.mark.parametrize("name", list(REGRESSIONS))
def test_regression_program(name):
    profile, seed, ops = REGRESSIONS[name]
    st = cs.State(profile)
    for op in ops:
        st.apply(op)                       # legal
    _run(ops, profile, seed)

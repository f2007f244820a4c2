"""
CPU tests of tests/call_sequences.py: the committed programs oracle against oracle, what they cover, and that the runner's checks can
fail (what tests/test_parity_helpers.py does for tests/parity.py).  The GPU runs the same programs in tests/test_gpu_call_sequences.py.
RDV_SEQ=profile:seed[:upto] restricts (a) to one program, cut after ``upto`` ops.
"""
import os

import pytest

import call_sequences as cs
from helpers import shipped_policy
from oracle_engine import OracleEngine, OracleModel

torch = pytest.importorskip("torch")

SELECTED = os.environ.get("RDV_SEQ")
PROGRAMS = [cs.parse_selection(SELECTED)[:2]] if SELECTED else cs.all_programs()
UPTO = cs.parse_selection(SELECTED)[2] if SELECTED else None


def _run(profile, seed, engine=OracleEngine, upto=None):
    n, params, kw = cs.engine_kwargs(profile, seed)
    return cs.run(cs.program(profile, seed), engine(n, params, **kw), OracleModel(n, params, **kw), upto=upto, profile=profile, seed=seed,
                  policy=shipped_policy(noise_seed=seed))


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("profile,seed", PROGRAMS, ids=[f"{p}:{s}" for p, s in PROGRAMS])
def test_program_is_legal_and_the_reference_alone_stays_inside_every_tolerance(profile, seed):
    """Every committed program (all seeds of every profile, general included) with the oracle as the subject: the generator's State
    asserts the legality of each op, and the comparisons of the runner all pass with nothing but the reference on both sides."""
    ops = cs.program(profile, seed)
    assert ops == cs.program(profile, seed), "program() is not deterministic"
    assert len(ops) <= cs.MAX_OPS
    st = cs.State(profile)
    for op in ops:
        st.apply(op)
    assert st.steps <= cs.MAX_ENV_STEPS
    _run(profile, seed, upto=UPTO)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("profile", list(cs.PROFILES))
def test_every_consumer_changer_consumer_triple_occurs(profile):
    """From the generator alone: every (X, C, Y) of legal_triples(profile) occurs in a committed program with nothing but changers
    between X and Y."""
    seeds = cs.SEEDS[profile]
    assert len(seeds) <= 12 and len({s % len(seeds) for s in seeds}) == len(seeds), "one seed per slice of the covering list"
    seen = set()
    for seed in seeds:
        seen |= cs.covered_triples(cs.program(profile, seed))
    want = set(cs.legal_triples(profile))
    assert len(want) == 9 * len(cs.changers(profile))
    missing = sorted(want - seen)
    print(f"{profile}: {len(want)} triples, {len(want & seen)} covered by {len(seeds)} programs")
    assert not missing, f"{profile}: {len(missing)} of {len(want)} triples never occur: {missing}"


@pytest.mark.parametrize("profile", list(cs.PROFILES))
def test_every_dispatchable_kernel_is_reached(profile):
    """The GPU test checks the kernel name after every consumer against State.kernel; here, from the generator and the same rules: every
    name the rules can produce for the profile is the expected name of at least one consumer, so the matrix cannot collapse onto one
    kernel silently."""
    seen = set()
    for seed in cs.SEEDS[profile]:
        seen |= set(cs.program_kernels(profile, seed))
    missing = sorted(cs.dispatchable_kernels(profile) - seen)
    assert not missing, f"{profile}: no consumer of a committed program launches {missing}"


def test_the_vocabulary_is_used():
    """Every op name, mask kind, state kind, variant, body, layout and pool set occurs in the committed programs."""
    used = {}
    for profile, seed in cs.all_programs():
        for op in cs.program(profile, seed):
            used.setdefault(op[0], set()).add(op[1:])
    names = set(cs.CONSUMERS) | {c for p in cs.PROFILES for c in cs.changers(p)} | {"eval_begin"}
    assert set(used) == names, set(used) ^ names
    first = lambda name: {a[0] for a in used[name]}
    assert first("reset_mask") == set(cs.MASKS) and first("set_state") == set(cs.STATE_KINDS) and first("variant") == set(cs.VARIANTS)
    assert first("step_many") == set(cs.KS) and first("rollout") == set(cs.KS) and first("tape_on") == {1, 2, 3}
    assert first("rigid_on") == set(range(len(cs.bodies()))) and first("group_on") == set(range(len(cs.LAYOUTS)))
    assert first("set_params") | {0} == set(range(len(cs.pool())))    # (set 0 is the constructor's)
    assert first("snapshot") == first("restore") == {0, 1}


# ---------------------------------------------------------------------------------------------------------------- (c)
RESET_FIELDS = ("nominal_rc0", "nominal_vc0", "nominal_qc0", "nominal_wc0", "nominal_qt0", "nominal_wt0", "rc0_range", "vc0_range",
                "qc0_range", "wc0_range", "qt0_range", "wt0_range")


class LateResetParams(OracleEngine):
    """set_params takes effect for resets only after the next full reset"""
    pending = None

    def set_params(self, params):
        late = params.copy()
        for f in RESET_FIELDS:
            setattr(late, f, getattr(self.params, f))
        self.pending = params
        super().set_params(late)

    def reset(self, mask=None):
        if mask is None and self.pending is not None:
            super().set_params(self.pending)
            self.pending = None
        return super().reset(mask)


class SeedIgnored(OracleEngine):
    def seed(self, seed):
        self._orc.seed(self._orc._seed)


class TapeOffIgnored(OracleEngine):
    def set_reset_tape(self, tape):
        if tape is not None:
            super().set_reset_tape(tape)


class MaskComplement(OracleEngine):
    def reset(self, mask=None):
        return super().reset(None if mask is None else 1 - mask)


class RestoreKeepsStatistics(OracleEngine):
    def restore(self, snap):
        self._orc.restore(snap, stats=False)
        self.obs = self.observe()


class SetStateNormalises(OracleEngine):
    def set_state(self, states):
        s = states.clone()
        for c in (slice(6, 10), slice(13, 17)):
            s[:, c] /= s[:, c].norm(dim=1, keepdim=True)
        super().set_state(s)


class GroupOffKeepsLastGroup(OracleEngine):
    def set_param_groups(self, params, group_sizes):
        if not len(params) and self._orc.groups is not None:
            self._orc.params = self._orc.groups[0][-1].copy()
        super().set_param_groups(params, group_sizes)


DEFECTS = [(LateResetParams, "set_params"), (SeedIgnored, "seed"), (TapeOffIgnored, "tape_off"), (MaskComplement, "reset_mask"),
           (RestoreKeepsStatistics, "restore"), (SetStateNormalises, "set_state"), (GroupOffKeepsLastGroup, "group_off")]


@pytest.mark.parametrize("engine,op", DEFECTS, ids=[e.__name__ for e, _ in DEFECTS])
def test_a_subject_with_one_defect_fails_a_committed_program(engine, op):
    """Each defective subject runs the committed programs of the profiles whose programs hold its op until one fails; the failure names
    the op it stopped at, and the defect's op lies in the program up to there."""
    profiles = ["groups"] if op == "group_off" else ["reset-f64", "tiny", "halt-f32", "groups"]
    for profile in profiles:
        for seed in cs.SEEDS[profile]:
            ops = cs.program(profile, seed)
            if not any(o[0] == op for o in ops):
                continue
            try:
                _run(profile, seed, engine=engine)
            except AssertionError as e:
                msg = str(e)
                assert f"RDV_SEQ={profile}:{seed} fails at" in msg and "the program up to it" in msg
                head = msg.split("\n")[0]
                print(engine.__name__, "->", head)
                at = int(head.split("fails at op ")[1].split(" ")[0]) if "fails at op " in head else len(ops) - 1
                assert any(o[0] == op for o in ops[:at + 1]), f"failed before the first {op}: {head}"
                return
    pytest.fail(f"{engine.__name__}: every committed program passed")

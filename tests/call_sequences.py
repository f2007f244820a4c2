"""Seeded random call sequences over the handle API (host only: no GPU, torch imported inside the runner).

A handle is a state machine: host flags (fresh, raw_state, prepared_ok, general, n_groups, variant, tape, seed) and per-env slot tags
decide which kernel a call launches and whether the persistent kernels may trust their prepared next-episode states.  The oracle
(tests/oracle_engine.py::OracleModel) has no such state: it draws every reset when it happens.  A PROGRAM is a list of plain tuples —
consumers (calls that step) and changers (calls that change what a later step or reset returns) — generated from
np.random.default_rng for a (profile, seed), legal by the rules of include/rdv.h; ``run`` executes it on a subject, on the model and,
if given, on a twin (a second handle that only ever takes plain steps), and compares after every op.

  python -m pytest tests/test_gpu_call_sequences.py -m gpu         with RDV_SEQ=profile:seed[:upto] runs one program, cut after
  ``upto`` ops: how a failing program is shortened by hand.
"""
import copy
import zlib

import numpy as np

import parity
import rigid_cases
from helpers import counter_actions, expected_kernel, oracle_batch, persistent_kernel, to_numpy
from reinforcement_learning_rendezvous_amd.params import GROUP_TILE, group_tile_table, make_params

LAYOUTS = ([256, 589], [512, 333], [256, 256, 333])
PROFILES = {
    "reset-f32": dict(storage="f32", on_done="reset", n=777),       # n % 4 != 0: obs_tmp rows, a ragged last wave
    "reset-f64": dict(storage="f64", on_done="reset", n=300),
    "halt-f32": dict(storage="f32", on_done="halt", n=333),         # with step_accumulate
    "continue-f32": dict(storage="f32", on_done="continue", n=260),
    "tiny": dict(storage="f32", on_done="reset", n=65),             # one lane into the second wave
    "groups": dict(storage="f32", on_done="reset", n=845),          # 256 + 512 + 77: LAYOUTS and back to ungrouped
    "general": dict(storage="f64", on_done="reset", n=130),         # BODIES on and off
}
# program(profile, seed) is built around the triples order[seed % len(SEEDS[profile]) :: len(SEEDS[profile])] of its profile, so the seeds
# of a profile have distinct residues, and a seed is replaced by one of the same residue.  Eight seeds do not cover the 108 triples of a
# plain profile within 40 ops (the enabling calls and the forced full resets cost ops too): ten do, and twelve cover the 135 triples of
# groups and the 126 of general.
SEEDS = {
    "reset-f32": (20, 21, 22, 23, 24, 25, 26, 27, 28, 29),
    "reset-f64": (20, 21, 22, 23, 24, 25, 26, 27, 28, 29),
    "halt-f32": (20, 21, 22, 23, 24, 25, 26, 27, 28, 29),
    "continue-f32": (20, 21, 22, 23, 24, 25, 26, 27, 28, 29),
    "tiny": (20, 21, 22, 23, 24, 25, 26, 27, 28, 29),
    "groups": (24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35),
    "general": (24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35),
}
MAX_OPS, MAX_ENV_STEPS = 40, 120
KS = (1, 2, 5, 9)
VARIANTS = ("auto", "fused", "split", "fused_inlane", "fused_tiles")
MASKS = ("random20", "none", "all", "env0", "last", "every5th")
STATE_KINDS = ("unnormalised", "in_koz", "other_env")
TRIPLE_CONSUMERS = ("step", "step_many", "rollout")
CONSUMERS = TRIPLE_CONSUMERS + ("step_diag", "step_accumulate", "act_step")
BASE_CHANGERS = ("reset_full", "reset_mask", "set_state", "set_params", "seed", "tape_on", "tape_off", "snapshot", "restore", "clone",
                 "variant", "stats_reset")


def changers(profile):
    return BASE_CHANGERS + {"groups": ("set_group_params", "group_on", "group_off"), "general": ("rigid_on", "rigid_off")}.get(profile, ())


_POOL = None


def pool():
    """Parameter sets under which every reason to end an episode occurs within a few steps: the time limit after 1, 2, 5 or 7 s, initial
    speeds outside the observation box, a nominal start inside the keep-out zone (CASES[5] of tests/test_gpu_slots.py), a target that
    turns the corridor away (attitude, bubble); other reset distributions, other reward coefficients, and dt = 0.5 (the last)."""
    global _POOL
    if _POOL is None:
        _POOL = [
            make_params(t_max=5.0),
            make_params(t_max=1.0),
            make_params(t_max=2.0, rc0_range=2.0, qt0_range=np.radians(10.0)),
            make_params(t_max=7.0, rc0=np.array([0.0, -2.6, 0.0]), rc0_range=1.5, koz_radius=4.0),
            make_params(t_max=5.0, reward_kwargs=dict(collision_coef=0.7, bonus_coef=6.0, fuel_coef=0.3, att_coef=1.2)),
            make_params(t_max=7.0, vc0_range=6.0, wc0_range=np.radians(8.0), wt0=np.radians([1.0, -2.0, 0.5]), wt0_range=np.radians(4.0)),
            make_params(t_max=2.0, dt=0.5, qc0_range=np.radians(25.0)),
        ]
    return _POOL


_BODIES = None


def bodies():
    """(keyword arguments of set_rigid_body, which body the RK45 integrates) from tests/rigid_cases.py; all four body arguments are
    always given, so that a switch from one body to another leaves nothing of the first."""
    global _BODIES
    if _BODIES is None:
        _BODIES = []
        for j, config in enumerate(("target", "chaser", "both", "forced")):
            kw = body_off()
            kw.update(rigid_cases.RigidCase(config, 1, "f64", "reset", seed=900 + j).body)
            _BODIES.append((kw, "chaser" if config == "chaser" else "target"))
    return _BODIES


def body_off():
    return dict(inertia=rigid_cases.REFERENCE_INERTIA.copy(), inertia_target=rigid_cases.REFERENCE_INERTIA.copy(), torque=np.zeros(3),
                torque_target=np.zeros(3), integrator="auto")


# ------------------------------------------------------------------------------------------------------------- legality state
class State:
    """What include/rdv.h lets the next call be, and which kernel it launches: tracked from the ops alone."""

    def __init__(self, profile):
        self.profile, self.p = profile, PROFILES[profile]
        self.tiles = -(-self.p["n"] // GROUP_TILE)
        self.variant, self.tape, self.raw = "auto", False, False
        self.layout, self.gparams, self.general, self.single = None, None, None, 0
        self.fresh, self.need_full, self.regs, self.eval, self.steps = True, True, set(), False, 0

    def tile_dt(self):
        if self.layout is None:
            return [pool()[self.single].dt] * self.tiles
        return [pool()[self.gparams[g]].dt for g in group_tile_table(self.p["n"], LAYOUTS[self.layout])]

    def legal(self, op):
        name = op[0]
        if self.need_full:                                  # after rdv_seed (and, here, a change of dt) the next reset is a full one
            return name == "reset_full" or (self.fresh and name in ("rigid_on", "rigid_off", "group_on", "group_off", "variant"))
        return {"set_params": self.layout is None, "set_group_params": self.layout is not None, "tape_off": self.tape,
                "restore": len(op) > 1 and op[1] in self.regs, "rigid_on": self.layout is None, "rigid_off": self.general is not None,
                "group_on": self.general is None, "group_off": self.layout is not None,
                "step_accumulate": self.p["on_done"] == "halt" and self.eval, "eval_begin": self.p["on_done"] == "halt",
                }.get(name, True)

    def kernel(self, op):
        """The name rdv_debug_last_kernel must give after consumer ``op`` (helpers.expected_kernel / persistent_kernel)."""
        name, p = op[0], self.p
        kw = dict(variant=self.variant, n=p["n"], on_done=p["on_done"], tape=self.tape, after_set_state=self.raw,
                  groups=self.layout is not None, general=self.general)
        if name in ("step_many", "rollout"):
            return persistent_kernel(name, p["storage"], n_steps=op[1], **kw)
        return expected_kernel(storage=p["storage"], diag=name in ("step_diag", "step_accumulate"), **kw)

    def apply(self, op):
        assert self.legal(op), (op, vars(self))
        name, dt0 = op[0], self.tile_dt()
        if name in CONSUMERS:
            self.steps += op[1] if name in ("step_many", "rollout") else 1
            self.raw = False
        elif name == "reset_full":
            self.fresh = self.need_full = False
        elif name in ("set_state", "restore"):
            self.raw = True
        elif name == "clone":
            self.raw, self.eval = True, False                # a clone is restored from a snapshot; its accumulators are not begun
        elif name == "set_params":
            self.single = op[1]
        elif name == "set_group_params":
            self.gparams = tuple(op[2] if g == op[1] else i for g, i in enumerate(self.gparams))
        elif name == "seed":
            self.fresh = self.need_full = True
        elif name in ("tape_on", "tape_off"):
            self.tape = name == "tape_on"
        elif name == "snapshot":
            self.regs.add(op[1])
        elif name == "variant":
            self.variant = op[1]
        elif name in ("rigid_on", "rigid_off"):
            self.general = bodies()[op[1]][1] if name == "rigid_on" else None
        elif name == "group_on":
            self.layout, self.gparams = op[1], tuple(op[2])
        elif name == "group_off":
            self.layout = self.gparams = None
        elif name == "eval_begin":
            self.eval = True
        if self.tile_dt() != dt0:
            # rdv.h defines no change of dt inside an episode (the reference keeps t, the library the step count): a full reset follows,
            # and no snapshot of the old time base is restored later
            self.need_full, self.regs = True, set()


# ------------------------------------------------------------------------------------------------------------- programs
def legal_triples(profile):
    """(X, C, Y): consumer, changer, consumer.  Every consumer is legal in every profile; the changers are the profile's."""
    return [(x, c, y) for c in changers(profile) for x in TRIPLE_CONSUMERS for y in TRIPLE_CONSUMERS]


def covered_triples(ops):
    """The triples (X, C, Y) of a program: X and Y consumers of TRIPLE_CONSUMERS with nothing but changers between them, C any of those."""
    out, last, between = set(), None, []
    for op in ops:
        name = op[0]
        if name in CONSUMERS:
            if last is not None and name in TRIPLE_CONSUMERS:
                out.update((last, c, name) for c in between)
            last, between = (name if name in TRIPLE_CONSUMERS else None), []
        elif name == "eval_begin":                          # neither: it ends the chain
            last = None
        else:
            between.append(name)
    return out


def program(profile, seed):
    """About 30 ops, at most MAX_OPS and MAX_ENV_STEPS env steps.  Plain random choice does not cover the profile's triples in 8 x 30
    ops, so a program is built around its share of a shuffled covering list (the same shuffle for every seed, one slice per seed), chained
    so that the Y of one triple is the X of the next, with random filler behind it."""
    crc = zlib.crc32(profile.encode())
    order = legal_triples(profile)
    np.random.default_rng(crc).shuffle(order)
    want = [tuple(t) for t in order[seed % len(SEEDS[profile])::len(SEEDS[profile])]]
    rng = np.random.default_rng([crc, seed])
    st, ops = State(profile), []
    pick = lambda xs: xs[int(rng.integers(len(xs)))]

    def emit(op, follow=True):
        ops.append(op)
        st.apply(op)
        if follow and st.need_full:                          # after seed, and after a change of dt
            ops.append(("reset_full",))
            st.apply(("reset_full",))

    def consumer(name):
        left = MAX_ENV_STEPS - st.steps
        k = pick([k for k in KS if k <= max(1, left // 4)])
        return {"step_many": ("step_many", k), "rollout": ("rollout", k, bool(rng.integers(2))),
                "act_step": ("act_step", bool(rng.integers(2)))}.get(name, (name,))

    def other_params(cur, same_dt):
        idx = [i for i in range(len(pool())) if i != cur and same_dt == (pool()[i].dt == pool()[cur].dt)]
        return pick(idx or [i for i in range(len(pool())) if i != cur])

    def group_on():
        li = pick([i for i in range(len(LAYOUTS)) if i != st.layout])
        return ("group_on", li, tuple(int(rng.integers(len(pool()) - (rng.random() < 0.8))) for _ in LAYOUTS[li]))

    def changer(name):
        s = int(rng.integers(1, 1 << 20))
        if name == "reset_mask":
            return (name, pick(MASKS), s)
        if name == "set_state":
            return (name, pick(STATE_KINDS), s)
        if name == "set_params":
            return (name, other_params(st.single, rng.random() < 0.75))
        if name == "set_group_params":
            g = int(rng.integers(len(st.gparams)))
            return (name, g, other_params(st.gparams[g], True))
        if name == "seed":
            return (name, s)
        if name == "tape_on":
            return (name, int(rng.integers(1, 4)), s)
        if name == "snapshot":
            return (name, int(rng.integers(2)))
        if name == "restore":
            return (name, pick(sorted(st.regs)))
        if name == "variant":
            return (name, pick([v for v in VARIANTS if v != st.variant]))
        if name == "rigid_on":
            return (name, int(rng.integers(len(bodies()))))
        if name == "group_on":
            return group_on()
        return (name,)

    enabler = {"set_params": "group_off", "set_group_params": "group_on", "tape_off": "tape_on", "restore": "snapshot",
               "rigid_off": "rigid_on", "group_off": "group_on"}

    def emit_changer(name):
        if not st.legal((name, min(st.regs) if st.regs else -1)):
            emit(changer(enabler[name]))
        emit(changer(name))

    # prologue: half of the groups / general programs start grouped / general
    if profile == "general" and rng.random() < 0.5:
        emit(changer("rigid_on"), follow=False)
    if profile == "groups" and rng.random() < 0.5:
        emit(group_on(), follow=False)
    emit(("reset_full",))
    def attempt(fn, limit):
        """fn() emits ops; undone if the program would grow beyond ``limit`` ops or the step budget"""
        nonlocal want, last
        keep = (len(ops), copy.deepcopy(st.__dict__), list(want), last, rng.bit_generator.state)
        fn()
        if len(ops) <= limit and st.steps <= MAX_ENV_STEPS:
            return True
        del ops[keep[0]:]
        st.__dict__, want, last, rng.bit_generator.state = keep[1], keep[2], keep[3], keep[4]
        return False

    special = ["step_diag", "act_step"] + (["step_accumulate"] if st.p["on_done"] == "halt" else [])

    def emit_special(name):
        if name == "step_accumulate" and not st.eval:
            emit(("eval_begin",))
        emit(consumer(name))

    def one_triple():
        nonlocal want, last
        cands = [t for t in want if t[0] == last]
        if not cands:
            last = max(TRIPLE_CONSUMERS, key=lambda x: sum(t[0] == x for t in want))
            emit(consumer(last))
            return
        follows = lambda t: sum(u[0] == t[2] and u != t for u in want)
        best = max((st.legal((t[1], min(st.regs) if st.regs else -1)), follows(t)) for t in cands)
        x, c, y = pick([t for t in cands if (st.legal((t[1], min(st.regs) if st.regs else -1)), follows(t)) == best])
        at = len(ops)
        emit_changer(c)
        emit(consumer(y))
        done = covered_triples([(x,)] + ops[at:])
        want = [t for t in want if t not in done]
        last = y

    # one consumer outside the triples in front of the chain, the chain, then pairs (changer, consumer outside the triples) behind it:
    # the evaluator build, its raw form (directly behind set_state / restore / clone), accumulate, act_step, every variant's plain step
    last = None
    emit_special(pick(special))
    while want and attempt(one_triple, MAX_OPS - 4):
        pass

    def tail():
        kind = pick(["raw_diag", "special", "variant_step", "special"])
        if kind == "raw_diag":
            emit_changer(pick(["set_state", "restore", "clone"]))
            emit(consumer("step_diag"))
        elif kind == "variant_step":
            if st.tape and rng.random() < 0.7:
                emit(("tape_off",))
            if st.general is not None and rng.random() < 0.5:
                emit(("rigid_off",))
            if st.layout is not None and rng.random() < 0.5:
                emit(("group_off",))
            emit(changer("variant"))
            emit(consumer("step"))
        else:
            if rng.random() < 0.5:
                emit_changer(pick([c for c in changers(profile) if c != "seed"]))
            emit_special(pick(special))

    misses, target = 0, min(MAX_OPS, max(30, len(ops) + 5))
    while len(ops) < target and misses < 4:
        misses += not attempt(tail, target)
    return ops


def parse_selection(text):
    """RDV_SEQ=profile:seed[:upto] -> (profile, seed, upto or None)."""
    parts = text.split(":")
    return parts[0], int(parts[1]), int(parts[2]) if len(parts) > 2 else None


def all_programs():
    return [(profile, seed) for profile in PROFILES for seed in SEEDS[profile]]


def dispatchable_kernels(profile):
    """Every kernel name the dispatch rules can produce for a profile: its storage and mode under every variant, with and without a
    reset tape, the evaluator build, the first step after rdv_set_state, its groups / bodies, and the persistent kernels."""
    st, out = State(profile), set()
    generals = [None] + (["target", "chaser"] if profile == "general" else [])
    for st.variant in VARIANTS:
        for st.tape in (False, True):
            for st.raw in (False, True):
                for st.general in generals:
                    for st.layout in [None] + ([0] if profile == "groups" else []):
                        for op in (("step",), ("step_diag",), ("step_many", 1), ("step_many", 2), ("rollout", 2, False)):
                            out.add(st.kernel(op))
    return out


def program_kernels(profile, seed):
    st, out = State(profile), []
    for op in program(profile, seed):
        if op[0] in CONSUMERS:
            out.append(st.kernel(op))
        st.apply(op)
    return out


# ------------------------------------------------------------------------------------------------------------- the runner
class _Rows:
    """One row of a step_many output behind the attributes parity.check_outputs reads off an env."""

    def __init__(self, env, done_reason):
        self._ctor, self.num_envs, self.done_reason = env._ctor, env.num_envs, done_reason


def _mask(kind, s, n):
    m = np.zeros(n, np.uint8)
    if kind == "random20":
        m[:] = np.random.default_rng(s).random(n) < 0.2
    elif kind == "all":
        m[:] = 1
    elif kind == "env0":
        m[0] = 1
    elif kind == "last":
        m[-1] = 1
    elif kind == "every5th":
        m[::5] = 1
    return m


def _states(base, kind, s):
    """The current state with about a third of the rows (row 0 always) replaced."""
    rng = np.random.default_rng(s)
    n = base.shape[0]
    rows = rng.random(n) < 0.3
    rows[0] = True
    m = int(rows.sum())
    out = base.copy()
    if kind == "unnormalised":                              # quaternions scaled by 0.5 to 3, chaser and target independently
        out[rows, 6:10] *= rng.uniform(0.5, 3.0, (m, 1))
        out[rows, 13:17] *= rng.uniform(0.5, 3.0, (m, 1))
    elif kind == "in_koz":                                  # the chaser 0.5 to 2.5 m from the target: inside every pool set's keep-out zone
        v = rng.normal(size=(m, 3))
        out[rows, 0:3] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.5, (m, 1))
    else:                                                   # rows of another env
        out[rows] = np.roll(base, 7, axis=0)[rows]
    return out


def _tape(depth, s, n):
    """States the oracle draws from another seed: every tape is a valid input."""
    rows = []
    for d in range(depth):
        o = oracle_batch(n, pool()[d % 3], "f64", "reset", seed=s + d)
        o.reset()
        rows.append(o.get_state())
    return np.stack(rows)


class _Run:
    def __init__(self, profile, seed, subject, model, twin, policy, twin_policy):
        import torch
        self.torch, self.profile, self.seed = torch, profile, seed
        self.p, self.st = PROFILES[profile], State(profile)
        self.subject, self.model, self.twin, self.policy, self.twin_policy = subject, model, twin, policy, twin_policy
        self.t, self.regs, self.kernels = 0, {}, []

    # ---- comparisons
    def engines(self):
        return [self.subject] + ([self.twin] if self.twin is not None else [])

    def same(self, a, b, what):
        t = self.torch
        ok = t.equal(a, b) if not a.is_floating_point() else bool(((a == b) | (t.isnan(a) & t.isnan(b))).all())
        assert ok, f"twin: {what}, step {self.t}"

    def same_state(self):
        if self.twin is not None:
            self.same(self.subject.get_state(), self.twin.get_state(), "state")
            self.same(self.subject.get_aux(), self.twin.get_aux(), "aux")

    def check_state(self, ref=None):
        s = self.subject
        if ref is not None:                                 # the evaluator's numbers of the state a training-path step left, where it is that state
            parity.check_diag(s, self.model, parity.live_rows(s, ref), self.t, False)
        parity.check_state(s, self.model, self.p["storage"], self.t)
        self.same_state()

    def check_after_changer(self):
        # parity.OBS_TOL, not RESET_OBS_TOL: the observed state has step arithmetic behind it
        np.testing.assert_allclose(to_numpy(self.subject.observe()), self.model.observe(), rtol=0, atol=parity.OBS_TOL, err_msg="observe()")
        self.check_state()
        if self.twin is not None:
            self.same(self.subject.observe(), self.twin.observe(), "observe()")

    def check_stats(self):
        parity.check_stats(self.subject, self.model, sums=True)
        if self.twin is not None:
            a, b = self.subject.get_stats(), self.twin.get_stats()
            assert a == b, f"twin: statistics {a} != {b}"

    def check_eval(self):
        got, want = to_numpy(self.subject.eval), self.model._acc
        counts = [1, 3, 6, 12, 17, 22, 27]                  # step / collision / success counts, level counts
        np.testing.assert_array_equal(got[:, counts], want[:, counts], err_msg="eval counts")
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="eval NaNs")
        # sums of per-step numbers that parity compares within DIAG_TOL each; the reward sum within RETURN_TOL, as an episode return
        np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=parity.RETURN_TOL, atol=parity.RETURN_TOL, err_msg="eval reward sum")
        np.testing.assert_allclose(got[:, 2:], want[:, 2:], rtol=parity.DIAG_TOL, atol=parity.DIAG_TOL, err_msg="eval sums")
        if self.twin is not None:
            self.same(self.subject.eval, self.twin.eval, "eval")

    # ---- consumers
    def actions(self, k):
        a = np.stack([counter_actions(self.seed, self.t + j, self.p["n"]) for j in range(k)])
        return a, self.torch.from_numpy(a).to(self.subject.device)

    def act(self, policy, env, obs, deterministic):
        if obs.is_cuda:
            return policy.act(obs, deterministic=deterministic, env_id_offset=env.env_id_offset).contiguous()
        from oracle_engine import cpu_act
        return cpu_act(policy, obs, deterministic)

    def one_step(self, a, a_t, diag=False, accumulate=False):
        s, w = self.subject, self.twin
        halted = self.model.halted()
        kw = dict(diag=True, accumulate=True) if accumulate else dict(diag=diag)
        o, r, d = s.step(a_t, **kw)
        ref = self.model.step(a, want_diag=diag, accumulate=accumulate)
        parity.check_outputs(s, ref, o, r, d, self.t)
        if diag or accumulate:
            parity.check_diag(s, ref, slice(None), self.t, True)
        if w is not None:
            w.step(a_t, **kw)
            for k in ("obs", "reward", "done", "done_reason"):
                self.same(getattr(s, k), getattr(w, k), k)
            new = s.done.bool() & ~self.torch.from_numpy(halted).to(s.device)
            for k in ("terminal_obs", "episode_return", "episode_length"):     # written where an episode ended
                self.same(getattr(s, k)[new], getattr(w, k)[new], k)
            if diag or accumulate:
                self.same(s.diag, w.diag, "diag")
        self.t += 1
        self.check_state(None if diag or accumulate else ref)
        if accumulate:
            self.check_eval()

    def op_step(self):
        a, a_t = self.actions(1)
        self.one_step(a[0], a_t[0])

    def op_step_diag(self):
        a, a_t = self.actions(1)
        self.one_step(a[0], a_t[0], diag=True)

    def op_step_accumulate(self):
        a, a_t = self.actions(1)
        self.one_step(a[0], a_t[0], accumulate=True)

    def op_act_step(self, deterministic):
        s, w = self.subject, self.twin
        a_t = self.act(self.policy, s, s.observe(), deterministic)
        if w is not None:
            self.same(a_t, self.act(self.twin_policy, w, w.observe(), deterministic), "policy actions")
        self.one_step(to_numpy(a_t), a_t)

    def op_step_many(self, k):
        s, w = self.subject, self.twin
        a, a_t = self.actions(k)
        out = s.step_many(a_t)
        for j in range(k):
            ref = self.model.step(a[j])
            parity.check_outputs(_Rows(s, out["done_reason"][j]), ref, out["obs"][j], out["reward"][j], out["done"][j], self.t, episode_rows=False)
            if w is not None:
                w.step(a_t[j])
                for key in ("obs", "reward", "done", "done_reason"):
                    self.same(out[key][j], getattr(w, key), f"step_many {key}")
            self.t += 1
        self.check_state(ref)

    def op_rollout(self, k, deterministic):
        s, w, torch = self.subject, self.twin, self.torch
        obs0 = self.model.observe()
        ro = s.rollout(self.policy, k, deterministic=deterministic)
        np.testing.assert_allclose(to_numpy(ro["obs"][0]), obs0, rtol=0, atol=parity.OBS_TOL, err_msg=f"rollout: first obs, step {self.t}")
        tobs = w.observe() if w is not None else None
        for j in range(k):
            # the clipped actions the subject's actor chose, replayed into the model (the actor's own numbers are pinned elsewhere)
            ref = self.model.step(np.clip(to_numpy(ro["actions"][j]), -1.0, 1.0))
            np.testing.assert_array_equal(to_numpy(ro["done"][j]), ref["done"], err_msg=f"rollout: done, step {self.t}")
            np.testing.assert_allclose(to_numpy(ro["reward"][j]), ref["reward"], rtol=parity.REWARD_TOL, atol=parity.REWARD_TOL,
                                       err_msg=f"rollout: reward, step {self.t}")
            nxt = ro["obs"][j + 1] if j + 1 < k else ro["last_obs"]
            np.testing.assert_allclose(to_numpy(nxt), ref["obs"], rtol=0, atol=parity.OBS_TOL, err_msg=f"rollout: obs, step {self.t}")
            if w is not None:
                self.same(ro["obs"][j], tobs, "rollout obs")
                ta = self.act(self.twin_policy, w, tobs, deterministic)
                self.same(torch.clamp(ro["actions"][j], -1.0, 1.0), ta, "rollout actions")
                tobs, r, d = w.step(ta)
                self.same(ro["reward"][j], r, "rollout reward")
                self.same(ro["done"][j], d, "rollout done")
            self.t += 1
        if w is not None:
            self.same(ro["last_obs"], tobs, "rollout last obs")
        self.check_state(ref)

    # ---- changers
    def op_reset_full(self):
        obs = [e.reset() for e in self.engines()]
        parity.check_reset_obs(obs[0], self.model.reset())

    def op_reset_mask(self, kind, s):
        m = _mask(kind, s, self.p["n"])
        for e in self.engines():
            e.reset(self.torch.from_numpy(m).to(e.device))
        self.model.reset(m)

    def op_set_state(self, kind, s):
        states = _states(self.model.get_state(), kind, s)
        for e in self.engines():
            e.set_state(self.torch.from_numpy(states))
        self.model.set_state(states)

    def op_set_params(self, i):
        for e in self.engines() + [self.model]:
            e.set_params(pool()[i])

    def op_set_group_params(self, g, i):
        for e in self.engines() + [self.model]:
            e.set_group_params(g, pool()[i])

    def op_seed(self, s):
        for e in self.engines() + [self.model]:
            e.seed(s)

    def op_tape_on(self, depth, s):
        tape = _tape(depth, s, self.p["n"])
        for e in self.engines():
            e.set_reset_tape(self.torch.from_numpy(tape))
        self.model.set_reset_tape(tape)

    def op_tape_off(self):
        for e in self.engines() + [self.model]:
            e.set_reset_tape(None)

    def op_snapshot(self, r):
        self.regs[r] = [e.snapshot() for e in self.engines() + [self.model]]

    def op_restore(self, r):
        for e, snap in zip(self.engines() + [self.model], self.regs[r]):
            e.restore(snap)

    def op_clone(self):
        """The run goes on with the clones; the originals are closed."""
        old = self.engines()
        self.subject = self.subject.clone()
        if self.twin is not None:
            self.twin = self.twin.clone()
        self.model = self.model.clone()
        for e in old:
            e.close()

    def op_variant(self, v):
        self.subject.set_kernel_variant(v)                  # the subject only: the twin stays on the in-lane layout

    def op_stats_reset(self):
        self.check_stats()
        for e in self.engines() + [self.model]:
            e.get_stats(reset=True)

    def op_rigid_on(self, j):
        from oracle_engine import rigid_from_kwargs
        kw = bodies()[j][0]
        for e in self.engines():
            e.set_rigid_body(**kw)
        self.model.set_rigid_body(rigid_from_kwargs(kw))

    def op_rigid_off(self):
        for e in self.engines():
            e.set_rigid_body(**body_off())
        self.model.set_rigid_body(None)

    def op_group_on(self, li, idx):
        params = [pool()[i] for i in idx]
        for e in self.engines():
            e.set_param_groups(params, LAYOUTS[li])
        self.model.group_on(params, LAYOUTS[li])

    def op_group_off(self):
        for e in self.engines():
            e.set_param_groups([], [])
        self.model.group_off()

    def op_eval_begin(self):
        for e in self.engines() + [self.model]:
            e.eval_begin()
        self.check_eval()

    def do(self, op):
        name = op[0]
        want = self.st.kernel(op) if name in CONSUMERS else None
        getattr(self, "op_" + name)(*op[1:])
        if want is not None and hasattr(self.subject, "last_kernel"):
            got = self.subject.last_kernel
            assert got == want, f"ran {got!r}, the dispatch rules say {want!r}"
            self.kernels.append(got)
        self.st.apply(op)
        if name not in CONSUMERS and name != "eval_begin" and not self.st.need_full:
            self.check_after_changer()
        if name == "stats_reset":
            self.check_stats()


def run(program, subject, model, twin=None, upto=None, *, profile, seed, policy=None, twin_policy=None):
    """Execute ``program[:upto]`` on every engine given and compare after every op (module docstring).  ``policy`` / ``twin_policy``: the
    actors of rollout and act_step, two objects with the same noise seed and call counter.  Returns the _Run: its subject and twin are
    the engines to close (clone replaces them), its kernels the names the subject's consumers launched."""
    ops = list(program if upto is None else program[:upto])
    r = _Run(profile, seed, subject, model, twin, policy, twin_policy)
    i = -1
    try:
        for i, op in enumerate(ops):
            r.do(op)
        i += 1
        if not r.st.fresh:
            r.check_stats()
    except AssertionError as e:
        listing = "\n".join(f"  {j:2d}: {o!r}" for j, o in enumerate(ops[:i + 1]))
        what = f"op {i} {ops[i]!r}" if i < len(ops) else "the statistics at the end"
        raise AssertionError(f"RDV_SEQ={profile}:{seed} fails at {what}; the program up to it:\n{listing}\n{e}") from None
    return r


def engine_kwargs(profile, seed):
    """The constructor arguments of a program's subject, twin and model: (n, first parameter set, keywords)."""
    p = PROFILES[profile]
    return p["n"], pool()[0], dict(storage=p["storage"], on_done=p["on_done"], seed=seed)

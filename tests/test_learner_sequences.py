"""
CPU tests of tests/learner_sequences.py: the committed programs are deterministic and legal, what they cover, and that the runner's
checks can fail — on ``FakeSet``, a pure-NumPy stand-in for a PolicySet that implements the documented semantics of the learner loop
(master rows the members' parameters are views of, re-viewed when a parameter's storage changed; blocks repacked by the step; moments
kept by update_weights, zeroed by reset_optimizer) and exposes only what the runner reads, with four switchable defects.  The GPU runs
the same programs on a real PolicySet in tests/test_gpu_learner_sequences.py.
RDV_LEARNER_SEQ=profile:seed[:upto] restricts the first test to one program, cut after ``upto`` ops.
"""
import os

import numpy as np
import pytest

import learner_sequences as L
import ppo_adam_reference as A

f32 = np.float32
SELECTED = os.environ.get("RDV_LEARNER_SEQ")
PROGRAMS = [L.parse_selection(SELECTED)[:2]] if SELECTED else L.all_programs()
UPTO = L.parse_selection(SELECTED)[2] if SELECTED else None
DEFECTS = {
    # name: (the kind of the op a failing program must stop at, the op that must lie in the program up to there)
    "reset_keeps_step": ("reset_opt", "reset_opt"),         # reset_optimizer zeroes the moments and keeps the step counter
    "replace_zeroes_moments": ("replace_member", "replace_member"),     # update_weights(member=, weights=) zeroes the member's moments
    "rebind_stale": ("step", "rebind"),                     # only the first parameter's storage is looked at: the step behind a rebind of
                                                            # another one leaves a stale tensor in state_dict()
    "skip_advances_step": ("step", "poison"),               # a skipped member's step counter advances
}


# ------------------------------------------------------------------------------------------------------------- the fake's "kernels"
def fake_forward(actor, critic, obs):
    """any function of all the weights and the rows, in float32"""
    act = np.tanh(obs @ actor[:102].reshape(17, 6)) + f32(actor.sum(dtype=np.float64))
    return act.astype(np.float32), (obs @ critic[:17] + f32(critic.sum(dtype=np.float64))).astype(np.float32)


def fake_grads(actor, critic, idx):
    s = f32(int((idx % 97).sum()) % 1000) / f32(1000)
    ga, gc = (np.sin(actor * f32(3) + s) * f32(0.01)).astype(np.float32), (np.cos(critic * f32(5) + s) * f32(0.02)).astype(np.float32)
    return ga, gc, np.array([ga.sum(), gc.sum(), s, 0, 0, 0], np.float32)


class FakeAlone:
    def __init__(self, profile, actor, critic):
        self.profile, self.w = profile, (np.array(actor, np.float32), np.array(critic, np.float32))

    def blocks(self):
        return tuple(x.copy() for x in self.w)

    def forward(self, g):
        return fake_forward(*self.w, L.fixed_obs(self.profile)[L.slices(self.profile)[g]])

    def grads(self, g, idx):
        return fake_grads(*self.w, idx)

    def close(self):
        pass


class FakeSet:
    """The learner loop's documented semantics on NumPy arrays.  ``params[g][k]``: the tensor member g's module holds for parameter k;
    after the first step they are NumPy views of the master rows, as the real parameters are views of the set's master weights."""

    def __init__(self, profile, defect=None):
        assert defect is None or defect in DEFECTS
        self.profile, self.defect, self.lay = profile, defect, L.layout(profile)
        self.P, self.n = len(L.PROFILES[profile]["sizes"]), len(self.lay)
        self.params = [[L.piece(profile, pair, k).copy() for k in range(self.n)] for pair in L.initial(profile)]
        self.blk = [self.flat(g) for g in range(self.P)]
        self.rows, self.ad, self.last, self.saved = None, None, None, None

    def flat(self, g):
        return tuple(np.concatenate([self.params[g][k].reshape(-1) for k, e in enumerate(self.lay) if e[1] == net]) for net in (0, 1))

    def close(self):
        pass

    # ---- the optimiser state
    def views(self):
        for g in range(self.P):
            pair = self.flat(g)
            for net in (0, 1):
                self.ad["master"][net][g] = pair[net]
            rows = (self.ad["master"][0][g], self.ad["master"][1][g])
            self.params[g] = [L.piece(self.profile, rows, k) for k in range(self.n)]

    def adam_state(self):
        if self.ad is None:
            z = lambda: [np.zeros((self.P, n), np.float32) for n in L.lengths(self.profile)]
            self.ad = dict(master=z(), m=z(), v=z(), step=np.zeros(self.P, np.int64), coef=np.zeros((self.P, 8), np.float32))
        looked_at = [0] if self.defect == "rebind_stale" else range(self.n)
        if not all(np.shares_memory(self.params[g][k], self.ad["master"][self.lay[k][1]][g]) for g in range(self.P) for k in looked_at):
            self.views()
        return self.ad

    # ---- what the runner reads
    def state(self, g):
        return self.flat(g)

    def blocks(self, g):
        return tuple(x.copy() for x in self.blk[g])

    def block_mismatch(self, got, want, actor):
        return None if L.bits(got, want) else "the blocks differ"

    def optimizer(self):
        if self.ad is None:
            return None
        return dict(m=[(self.ad["m"][0][g], self.ad["m"][1][g]) for g in range(self.P)],
                    v=[(self.ad["v"][0][g], self.ad["v"][1][g]) for g in range(self.P)], step=self.ad["step"])

    def alone(self, actor, critic):
        return FakeAlone(self.profile, actor, critic)

    # ---- consumers
    def forward(self):
        obs = L.fixed_obs(self.profile)
        parts = [fake_forward(*self.blk[g], obs[sl]) for g, sl in enumerate(L.slices(self.profile))]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def grads(self, idx):
        if self.rows is None:
            self.rows = [np.zeros((self.P, n), np.float32) for n in L.lengths(self.profile)]
        out = dict(rows=None, grad=[None] * self.P, scalars=[None] * self.P)
        self.last = [None] * self.P
        for g in range(self.P):
            if idx[g] is not None:
                ga, gc, out["scalars"][g] = fake_grads(*self.blk[g], idx[g])
                self.rows[0][g], self.rows[1][g] = ga, gc
                out["grad"][g], self.last[g] = (ga.copy(), gc.copy()), {}
        out["rows"] = [(self.rows[0][g].copy(), self.rows[1][g].copy()) for g in range(self.P)]
        return out

    def step(self, which, lr, max_norm, eps):
        ad = self.adam_state()
        for g in range(self.P) if which is None else which:
            ga, gc = self.rows[0][g], self.rows[1][g]
            if not (np.isfinite(ga).all() and np.isfinite(gc).all()):
                ad["coef"][g] = [np.nan, 0, 0, 0, 1, 0, 0, 0]
                ad["step"][g] += self.defect == "skip_advances_step"
                continue
            coef = A.coef32(ga, gc, int(ad["step"][g]), lr, L.B1, L.B2, max_norm)
            ad["coef"][g] = list(coef) + [0, 0, 0, 0]
            for net, grad in ((0, ga), (1, gc)):
                p, m, v = A.step32(ad["master"][net][g], ad["m"][net][g], ad["v"][net][g], grad, coef, L.B1, L.B2, eps)
                ad["master"][net][g], ad["m"][net][g], ad["v"][net][g] = p, m, v         # written into the rows: the views follow
            ad["step"][g] += 1
            self.blk[g] = tuple(ad["master"][net][g].copy() for net in (0, 1))             # the step repacks the member's blocks
        return ad["coef"].copy()

    # ---- changers
    def write(self, g, pair, ks=None):
        for k in range(self.n) if ks is None else ks:
            self.params[g][k][...] = L.piece(self.profile, pair, k)                        # in place: through the views

    def push_member(self, g):
        self.blk[g] = self.flat(g)

    def push(self):
        for g in range(self.P):
            self.push_member(g)

    def replace_member(self, g, actor, critic):
        self.write(g, (actor, critic))
        self.push_member(g)
        if self.defect == "replace_zeroes_moments" and self.ad is not None:
            for net in (0, 1):
                self.ad["m"][net][g], self.ad["v"][net][g] = 0, 0

    def replace_all(self, new):
        for g, pair in enumerate(new):
            if pair is not None:
                self.write(g, pair)
        self.push()

    def edit(self, g, how, actor, critic, ks):
        self.write(g, (actor, critic), None if how == "load" else ks)

    def reset_opt(self, g):
        if self.ad is not None:
            todo = list(range(self.P)) if g is None else [g]
            for net in (0, 1):
                self.ad["m"][net][todo], self.ad["v"][net][todo] = 0, 0
            if self.defect != "reset_keeps_step":
                self.ad["step"][todo] = 0

    def move_off(self):
        self.params = [[p.copy() for p in ps] for ps in self.params]                      # .to(): new storage for every parameter

    move_on = move_off

    def rebind(self, g, k, kind, values):
        self.params[g][k] = self.params[g][k].copy()
        if values is not None:
            self.params[g][k][...] = values

    def poison(self, g, net, j):
        self.rows[net][g, j] = np.nan

    def checkpoint(self):
        self.saved = [self.flat(g) for g in range(self.P)]

    def load_checkpoint(self, g):
        self.write(g, self.saved[g])
        return fake_forward(*self.saved[g], L.fixed_obs(self.profile)[L.slices(self.profile)[g]])


def _run(profile, seed, defect=None, upto=None):
    return L.run(L.program(profile, seed), FakeSet(profile, defect), upto=upto, profile=profile, seed=seed)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("profile,seed", PROGRAMS, ids=[f"{p}:{s}" for p, s in PROGRAMS])
def test_program_is_deterministic_and_legal_and_the_clean_fake_passes(profile, seed):
    ops = L.program(profile, seed)
    assert ops == L.program(profile, seed), "program() is not deterministic"
    assert 0 < len(ops) <= L.MAX_OPS
    st = L.State(profile)
    for op in ops:
        assert op[0] in L.CONSUMERS + L.CHANGERS
        st.apply(op)                                        # asserts the model's own rules
    r = _run(profile, seed, upto=UPTO)
    if UPTO is None:                                        # the run went somewhere: the optimiser state exists
        assert r.subject.ad is not None and any(op[0] == "step" for op in ops)


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("profile", list(L.PROFILES))
def test_every_changer_meets_every_consumer_and_precedes_a_step_behind_a_grads(profile):
    """From the generator alone: every (changer, consumer kind) occurs directly adjacent in a committed program, and every changer is
    directly followed by grads, step somewhere.  A condition on SEEDS, asserted here."""
    seeds = L.SEEDS[profile]
    assert len(seeds) <= 12 and len({s % len(seeds) for s in seeds}) == len(seeds), "one seed per slice of the covering list"
    seen, triples = set(), set()
    for seed in seeds:
        ops = L.program(profile, seed)
        seen |= L.covered_pairs(ops)
        triples |= L.covered_triples(ops)
    want = set(L.pairs())
    assert len(want) == 3 * len(L.CHANGERS) == 36
    assert not want - seen, f"{profile}: never adjacent: {sorted(want - seen)}"
    assert triples == set(L.CHANGERS), f"{profile}: never directly in front of grads, step: {sorted(set(L.CHANGERS) - triples)}"


def test_the_vocabulary_is_used():
    """Every op, every hyperparameter of the pool, both forms of step, edit, rebind and reset_opt; rebind over ALL parameters; changers
    in front of the first step as well as behind it."""
    for profile in L.PROFILES:
        used, before_first_step = {}, set()
        for seed in L.SEEDS[profile]:
            stepped = False
            for op in L.program(profile, seed):
                used.setdefault(op[0], set()).add(op[1:])
                stepped = stepped or op[0] == "step"
                if not stepped:
                    before_first_step.add(op[0])
        P, n = len(L.PROFILES[profile]["sizes"]), len(L.layout(profile))
        assert set(used) == set(L.CONSUMERS + L.CHANGERS)
        hypers = {a[1] for a in used["step"]}
        assert {h[0] for h in hypers} == {0, 1} and {h[1] for h in hypers} == {0, 1, 2} and {h[2] for h in hypers} == {0, 1}
        assert None in {a[0] for a in used["step"]} and (P == 1 or any(a[0] is not None and len(a[0]) < P for a in used["step"]))
        assert P == 1 or any(len(a[0]) < P for a in used["grads"]), "no member ever sits out"
        assert {a[1] for a in used["edit_in_place"]} == {"load", "copy"} and {a[2] for a in used["rebind"]} == {"data", "parameter"}
        ks = {a[1] for a in used["rebind"]}
        assert len(ks - {0}) >= 3 and max(ks) >= n // 2, f"{profile}: rebind reaches parameters {sorted(ks)} of {n}"
        assert {a[3] is None for a in used["rebind"]} == {True, False}
        assert None in {a[0] for a in used["reset_opt"]} and {a[0] for a in used["reset_opt"]} - {None}
        assert before_first_step & set(L.CHANGERS), f"{profile}: no changer in front of a first step"


def test_the_layout_is_the_flat_layout_of_the_reference():
    import policy_mlp_reference as M
    for profile, p in L.PROFILES.items():
        pair = L.initial(profile)[0]
        nets = L.nets_of(profile, pair)
        assert M.arch_of(nets[0]) == list(p["pi"]) and M.arch_of(nets[1]) == list(p["vf"])
        assert all(L.bits(A.flat(n), x) for n, x in zip(nets, pair))
        assert len(L.layout(profile)) == 2 * (len(p["pi"]) + len(p["vf"]) + 2) + 1
    assert L.lengths("shipped") == (A.ACTOR, A.CRITIC) and len(L.layout("shipped")) == 13
    idx = L.minibatch("shipped", 2, 5)
    assert idx.size in L.MB_SIZES and bool(((idx % 612 >= 512) & (idx < L.T * 612)).all()) and idx[idx.size // 2] == idx[1]


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_fake_with_one_defect_fails_a_committed_program_at_the_defects_op(defect):
    """Each defective fake runs the committed programs until one fails: the message names the profile, the seed and the op index, the
    failing op is of the defect's kind, the op that sets the defect off lies in the program up to there, and the program cut in front
    of the failing op passes."""
    kind, cause = DEFECTS[defect]
    for profile, seed in L.all_programs():
        ops = L.program(profile, seed)
        try:
            _run(profile, seed, defect)
        except AssertionError as e:
            head = str(e).split("\n")[0]
            print(defect, "->", head)
            assert head.startswith(f"RDV_LEARNER_SEQ={profile}:{seed}:") and "fails at op " in head and "the program up to it" in head
            at = int(head.split("fails at op ")[1].split(" ")[0])
            assert L.parse_selection(head.split("=")[1].split(" ")[0]) == (profile, seed, at + 1)
            assert ops[at][0] == kind, f"{defect}: failed at {ops[at]!r}, not at a {kind}"
            assert any(o[0] == cause for o in ops[:at + 1])
            _run(profile, seed, defect, upto=at)
            with pytest.raises(AssertionError, match=f"fails at op {at} "):
                _run(profile, seed, defect, upto=at + 1)
            return
    pytest.fail(f"{defect}: every committed program passed")

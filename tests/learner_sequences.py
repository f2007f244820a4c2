"""Seeded random call sequences over the learner loop of a PolicySet (host only at import: no GPU, torch imported inside the subject).

A ``PolicySet`` that has taken a device ``adam_step`` is a state machine: it owns fp32 master weights, moments and step counters, the
member modules' parameters are views of the master rows and their ``.grad`` views of the set's gradient rows, the forward blocks are
rewritten by the step itself, and ``.to()`` or new Parameter storage makes the modules the source of truth again
(reinforcement_learning_rendezvous_amd/ppo.py: ``_adam_state``, ``_adam_views``, ``_adam_device``).  The MODEL here has no such state.
Per member g it keeps plain NumPy arrays:

    mod[g]    flat actor / critic float32 vectors (the layout of ppo_adam_reference.flat): what the member's modules hold;
    blk[g]    the weights from which the set's forward blocks were last packed;
    m, v, step[g]   the optimiser state;   G[g]  the gradient row the set holds for g, or None;   coef[g]  its last coefficient row.

It contains no library code: the elementwise step is ppo_adam_reference.step32 (any row length) fed with the read-back ``coef``, whose
first four floats are held to ppo_adam_reference.coef64 within 1 ulp — the tolerance of tests/test_gpu_ppo_adam.py.

A PROGRAM is a list of plain tuples drawn from np.random.default_rng for a (profile, seed): consumers (``forward``, ``grads``, ``step``)
and changers (CHANGERS), legal by the rules of ``State``.  ``run`` executes it on a SUBJECT and on the model.  Consumers are compared
with stand-alone policies built from ``blk`` (the subject makes them: ``alone``), bit for bit; after EVERY op, for EVERY member:
``state_dict()`` equals ``mod`` as bits, both forward blocks equal those of a stand-alone policy of ``blk`` (the subject's
``block_mismatch``: ppo_adam_reference.blocks_equal), and the moments and step counters equal the model's once the subject has them.

The subject is anything with the methods ``SetSubject`` has: that class drives a real PolicySet on the GPU
(tests/test_gpu_learner_sequences.py); tests/test_learner_sequences.py runs the same programs on a NumPy fake with switchable defects.

    RDV_LEARNER_SEQ=profile:seed[:upto]    runs one program, cut after ``upto`` ops: how a failing program is shortened by hand.
"""
import zlib

import numpy as np

import ppo_adam_reference as A

f32 = np.float32
T = 4                                                       # steps of the buffer collected once at the start
B1, B2 = 0.9, 0.999
LRS, NORMS, EPSS = (3e-4, 1e-3), (0.5, float("inf"), 1e-3), (1e-5, 1e-8)
COEFS = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)    # of every ppo_grads / ppo_grad
MB_SIZES = (33, 128, 200)                                   # a partial wave; one 128-row workgroup; more than one
MAX_OPS = 40
PROFILES = {
    "shipped": dict(pi=(64, 64), vf=(64, 64), act="tanh", sizes=(256, 256, 100)),     # rdv_ppo_set_*
    "mlp": dict(pi=(16, 32), vf=(32,), act="relu", sizes=(256, 256, 100)),            # rdv_ppo_mlp_set_*
    "one": dict(pi=(64, 64), vf=(64, 64), act="tanh", sizes=(300,)),                  # a set of one member
}
# program(profile, seed) is built around the pairs order[seed % len(SEEDS[profile]) :: len(SEEDS[profile])] of its profile, so the seeds
# of a profile have distinct residues, and a seed is replaced by one of the same residue
SEEDS = {"shipped": (30, 31, 32, 33, 34, 35), "mlp": (30, 31, 32, 33, 34, 35), "one": (30, 31, 32, 33, 34, 35)}
CONSUMERS = ("forward", "grads", "step")
CHANGERS = ("push", "push_member", "replace_member", "replace_all", "edit_in_place", "reset_opt", "move_off", "move_on", "rebind", "poison",
            "checkpoint", "load_checkpoint")


# ------------------------------------------------------------------------------------------------------------- layouts and inputs
def layout(profile):
    """[(name, net, at, shape)] of a member's parameters in the order of the flat gradient rows (ppo._params): the actor's layers (w then
    b), log_std, the critic's layers; ``net`` 0: actor, 1: critic; ``at``: the offset in that net's flat vector."""
    p, out = PROFILES[profile], []
    for net, prefix, arch, head in ((0, "l", p["pi"], 6), (1, "v", p["vf"], 1)):
        dims, at = [17] + list(arch) + [head], 0
        for i in range(len(dims) - 1):
            out.append((f"{prefix}{i + 1}.weight", net, at, (dims[i + 1], dims[i]))); at += dims[i + 1] * dims[i]
            out.append((f"{prefix}{i + 1}.bias", net, at, (dims[i + 1],))); at += dims[i + 1]
        if net == 0:
            out.append(("log_std", 0, at, (6,)))
    return out


def lengths(profile):
    """(Ga, Gc): the lengths of a member's flat actor and critic vectors"""
    out = [0, 0]
    for _, net, at, shape in layout(profile):
        out[net] = max(out[net], at + int(np.prod(shape)))
    return tuple(out)


def piece(profile, flats, k):
    """parameter k of a member's flat pair, shaped (a view)"""
    _, net, at, shape = layout(profile)[k]
    return flats[net][at:at + int(np.prod(shape))].reshape(shape)


def nets_of(profile, flats):
    """(actor, critic) as policy_mlp_reference networks"""
    import policy_mlp_reference as M
    p, lay = PROFILES[profile], layout(profile)
    out = []
    for net in (0, 1):
        ks = [k for k, e in enumerate(lay) if e[1] == net and e[0] != "log_std"]
        ws, bs = [piece(profile, flats, k).copy() for k in ks[0::2]], [piece(profile, flats, k).copy() for k in ks[1::2]]
        log_std = piece(profile, flats, [e[0] for e in lay].index("log_std")).copy() if net == 0 else None
        out.append(M.make_net(ws, bs, p["act"], log_std))
    return tuple(out)


def weights_of(profile, flats):
    """the dict MlpPolicy and update_weights take"""
    import policy_mlp_reference as M
    return M.weights_dict(*nets_of(profile, flats))


def initial(profile):
    """The members' first weights as flat pairs: dense random nets with log_std in [-1.4, -0.4] (the recipe of
    ppo_reference.random_nets), seeds that differ by member so that a wrong member's row cannot pass."""
    import policy_mlp_reference as M
    p, out = PROFILES[profile], []
    for g in range(len(p["sizes"])):
        seed = 100 + 2 * g
        a = M.dense(list(p["pi"]), p["act"], seed=seed)
        a["log_std"] = np.random.default_rng([seed, 77]).uniform(-1.4, -0.4, size=6).astype(np.float32)
        out.append((A.flat(a), A.flat(M.critic_of(M.dense(list(p["vf"]), p["act"], seed=seed + 1)))))
    assert tuple(x.size for x in out[0]) == lengths(profile)
    return out


def perturbed(x, seed, rel):
    """x + rel * N(0, 1) * (|x| + 0.01) in float32"""
    x = np.asarray(x, np.float32)
    return (x + f32(rel) * np.random.default_rng([seed, 9]).standard_normal(x.shape).astype(np.float32) * (np.abs(x) + f32(0.01))).astype(np.float32)


def fixed_obs(profile):
    n = sum(PROFILES[profile]["sizes"])
    return np.random.default_rng([n, 3]).uniform(-1.0, 1.0, size=(n, 17)).astype(np.float32)


def slices(profile):
    starts = np.concatenate([[0], np.cumsum(PROFILES[profile]["sizes"])])
    return [slice(int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])]


def minibatch(profile, g, mb_seed):
    """Flat rows of member g's env columns of the [T, N] buffer: one of MB_SIZES shuffled rows, one of them twice."""
    sl, n_envs = slices(profile)[g], sum(PROFILES[profile]["sizes"])
    size = sl.stop - sl.start
    rng = np.random.default_rng([mb_seed, g])
    n = MB_SIZES[int(rng.integers(len(MB_SIZES)))]
    local = rng.permutation(T * size)[:n]
    idx = (local // size) * n_envs + sl.start + local % size
    idx[n // 2] = idx[1]
    return idx.astype(np.int64)


def hyper(h):
    return LRS[h[0]], NORMS[h[1]], EPSS[h[2]]


def bits(a, b):
    """equal as bits (so a NaN equals itself and -0 is not +0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- legality state
class State:
    """What the next op may be, tracked from the ops alone.  A ``step`` takes the device route only behind a device ``grads`` (sequences
    that mix the device optimiser and the PyTorch fallback are not drawn: their moments are different stores by design), so ``step``
    with the list the last ``grads`` returned needs that ``grads``, and ``step`` with None needs a gradient row for every member."""

    def __init__(self, profile):
        self.profile, self.P = profile, len(PROFILES[profile]["sizes"])
        self.has_g, self.last, self.on, self.ckpt, self.stepped = [False] * self.P, None, False, False, False

    def steps(self):
        """the legal ``which`` of a step"""
        return ([self.last] if self.last is not None else []) + ([None] if all(self.has_g) else [])

    def legal(self, op):
        name = op[0]
        if name == "step":
            return op[1] in self.steps()
        if name == "grads":
            return len(op[1]) > 0 and all(0 <= g < self.P for g in op[1])
        return {"poison": name == "poison" and self.has_g[op[1]], "move_off": self.on, "move_on": not self.on,
                "load_checkpoint": self.ckpt}.get(name, True)

    def apply(self, op):
        assert self.legal(op), (op, vars(self))
        name = op[0]
        if name == "grads":
            self.last = tuple(op[1])
            for g in op[1]:
                self.has_g[g] = True
        elif name == "step":
            self.on = self.stepped = True                   # the device step brings the modules to its device
        elif name in ("move_off", "move_on"):
            self.on = name == "move_on"
        elif name == "checkpoint":
            self.ckpt = True


# ------------------------------------------------------------------------------------------------------------- programs
def pairs():
    """(changer, consumer): every one occurs directly adjacent in a profile's programs; a (changer, grads) is followed by a step"""
    return [(c, y) for c in CHANGERS for y in CONSUMERS]


def covered_pairs(ops):
    return {(a[0], b[0]) for a, b in zip(ops, ops[1:]) if a[0] in CHANGERS and b[0] in CONSUMERS}


def covered_triples(ops):
    """the changers directly followed by grads, step"""
    return {a[0] for a, b, c in zip(ops, ops[1:], ops[2:]) if a[0] in CHANGERS and b[0] == "grads" and c[0] == "step"}


def program(profile, seed):
    """At most MAX_OPS ops: mostly a first grads + step (so that the device state exists), then this seed's share of the shuffled pairs
    (the same shuffle for every seed of the profile) with whatever makes them legal in front, then random filler."""
    crc = zlib.crc32(profile.encode())
    order = pairs()
    np.random.default_rng(crc).shuffle(order)
    n_seeds = len(SEEDS[profile])
    want = [tuple(t) for t in order[seed % n_seeds::n_seeds]]
    rng = np.random.default_rng([crc, seed])
    st, ops = State(profile), []
    P, n_params = st.P, len(layout(profile))
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    s = lambda: int(rng.integers(1, 1 << 20))

    def emit(op):
        ops.append(op)
        st.apply(op)

    def grads():
        live = tuple(g for g in range(P) if rng.random() < 0.7) or (int(rng.integers(P)),)
        return ("grads", live, s())

    def step(member=None):
        """a legal step, one that ``member`` takes if there is one"""
        cands = st.steps()
        with_member = [w for w in cands if w is None or member is None or member in w]
        return ("step", pick(with_member or cands), (int(rng.integers(2)), int(rng.integers(3)), int(rng.integers(2))))

    def changer(name, before_step=False):
        live = [g for g in range(P) if st.has_g[g] and (not before_step or st.last is None or g in st.last or all(st.has_g))]
        g = pick(live) if (name == "poison" or (before_step and live)) else int(rng.integers(P))
        if name == "replace_all":
            seeds = [s() for _ in range(P)]
            if P > 1:
                seeds[int(rng.integers(P))] = None
            return (name, tuple(seeds))
        if name in ("push_member", "load_checkpoint"):
            return (name, g)
        if name == "replace_member":
            return (name, g, s())
        if name == "edit_in_place":
            return (name, g, pick(["load", "copy"]), s())
        if name == "reset_opt":
            return (name, g if rng.random() < 0.5 else None)
        if name == "rebind":
            return (name, g, int(rng.integers(n_params)), pick(["data", "parameter"]), s() if rng.random() < 0.5 else None)
        if name == "poison":
            return (name, g, int(rng.integers(2)), s())
        return (name,)

    enabler = {"move_off": "move_on", "move_on": "move_off", "load_checkpoint": "checkpoint"}

    def emit_changer(name, before_step=False):
        if name == "poison":
            if not any(st.has_g):
                emit(grads())
        elif not st.legal((name, 0)):
            emit(changer(enabler[name]))
        op = changer(name, before_step)
        emit(op)
        return op[1] if len(op) > 1 and isinstance(op[1], int) else None

    def consumer(name, member=None):
        if name == "forward":
            return ("forward",)
        return grads() if name == "grads" else step(member)

    if seed % n_seeds:                                      # one program of a profile starts with its changers in front of any step
        emit(("grads", tuple(range(P)), s()))
        emit(step())
    for c, y in want:
        if y == "step" and not st.steps():
            emit(grads())
        member = emit_changer(c, before_step=y == "step")
        emit(consumer(y, member))
        if y == "grads":
            emit(step(member))
    assert len(ops) <= MAX_OPS - 2, (profile, seed, len(ops))
    target = min(MAX_OPS, max(32, len(ops) + 4))
    while len(ops) < target:
        name = pick(CONSUMERS + CHANGERS) if rng.random() < 0.6 else pick(CONSUMERS)
        if name == "step" and not st.steps():
            name = "grads"
        if name in CHANGERS:
            if name == "poison" and not any(st.has_g):
                continue
            if not st.legal((name, 0)) and name != "poison":
                continue
            emit(changer(name))
        else:
            emit(consumer(name))
    return ops


def parse_selection(text):
    """RDV_LEARNER_SEQ=profile:seed[:upto] -> (profile, seed, upto or None)."""
    parts = text.split(":")
    return parts[0], int(parts[1]), int(parts[2]) if len(parts) > 2 else None


def all_programs():
    return [(profile, seed) for profile in PROFILES for seed in SEEDS[profile]]


# ------------------------------------------------------------------------------------------------------------- the runner
class _Run:
    def __init__(self, profile, seed, subject):
        self.profile, self.seed, self.subject = profile, seed, subject
        self.P, self.st = len(PROFILES[profile]["sizes"]), State(profile)
        self.init = [tuple(x.copy() for x in pair) for pair in initial(profile)]
        self.mod = [[x.copy() for x in pair] for pair in self.init]
        self.blk = [[x.copy() for x in pair] for pair in self.init]
        zeros = lambda: [np.zeros(n, np.float32) for n in lengths(profile)]
        self.m, self.v, self.step = [zeros() for _ in range(self.P)], [zeros() for _ in range(self.P)], [0] * self.P
        self.G, self.coef, self.ckpt = [None] * self.P, [np.zeros(8, np.float32) for _ in range(self.P)], None
        self._alone = [None] * self.P                       # the stand-alone policy of blk[g], made when first needed, closed when blk[g] changes

    # ---- the stand-alone policies
    def set_blk(self, g, pair):
        self.blk[g] = [np.asarray(x, np.float32).copy() for x in pair]
        self.drop(g)

    def drop(self, g):
        if self._alone[g] is not None:
            self._alone[g]["policy"].close()
            self._alone[g] = None

    def alone(self, g):
        if self._alone[g] is None:
            policy = self.subject.alone(*self.blk[g])
            self._alone[g] = dict(policy=policy, blocks=None)
        return self._alone[g]["policy"]

    def want_blocks(self, g):
        policy = self.alone(g)
        if self._alone[g]["blocks"] is None:
            self._alone[g]["blocks"] = policy.blocks()
        return self._alone[g]["blocks"]

    def close(self):
        for g in range(self.P):
            self.drop(g)

    # ---- what holds after every op
    def check_all(self):
        s = self.subject
        for g in range(self.P):
            got = s.state(g)
            for k, net in enumerate(("actor", "critic")):
                if not bits(got[k], self.mod[g][k]):
                    at = np.flatnonzero(np.asarray(got[k], np.float32).view(np.uint32) != self.mod[g][k].view(np.uint32))
                    names = sorted({e[0] for e in layout(self.profile) if e[1] == k and any(e[2] <= i < e[2] + int(np.prod(e[3])) for i in at[:2000])})
                    raise AssertionError(f"member {g}: state_dict() is not the model's {net} weights: {at.size} floats differ, in {names}")
            blocks, want = s.blocks(g), self.want_blocks(g)
            for k, net in enumerate(("actor", "critic")):
                msg = s.block_mismatch(blocks[k], want[k], k == 0)
                assert msg is None, f"member {g}: the {net} block is not the block of the weights it was packed from: {msg}"
        opt = s.optimizer()
        if opt is not None:
            for g in range(self.P):
                assert int(opt["step"][g]) == self.step[g], f"member {g}: step counter {int(opt['step'][g])}, the model's is {self.step[g]}"
                for k, net in enumerate(("actor", "critic")):
                    assert bits(opt["m"][g][k], self.m[g][k]), f"member {g}: first moments of the {net}"
                    assert bits(opt["v"][g][k], self.v[g][k]), f"member {g}: second moments of the {net}"

    # ---- consumers
    def op_forward(self):
        act, val = self.subject.forward()
        for g, sl in enumerate(slices(self.profile)):
            a, v = self.alone(g).forward(g)
            assert bits(act[sl], a), f"forward: member {g}'s deterministic actions are not those of its block's weights"
            assert bits(val[sl], v), f"forward: member {g}'s values are not those of its block's weights"

    def op_grads(self, live, mb_seed):
        idx = [minibatch(self.profile, g, mb_seed) if g in live else None for g in range(self.P)]
        out = self.subject.grads(idx)
        for g in range(self.P):
            if g not in live:
                assert out["grad"][g] is None and out["scalars"][g] is None
                if self.G[g] is not None:
                    assert all(bits(x, y) for x, y in zip(out["rows"][g], self.G[g])), f"grads: the row of member {g}, which sat out, changed"
                continue
            ga, gc, scalars = self.alone(g).grads(g, idx[g])
            for k, (net, want) in enumerate((("actor", ga), ("critic", gc))):
                assert bits(out["rows"][g][k], want), f"grads: member {g}'s {net} row is not MlpPolicy.ppo_grad of its block's weights"
                assert bits(out["grad"][g][k], want), f"grads: member {g}'s {net} .grad is not its row"
            assert bits(out["scalars"][g], scalars), f"grads: member {g}'s scalars {out['scalars'][g]} != {scalars}"
            assert np.isfinite(ga).all() and np.isfinite(gc).all() and float(np.abs(ga).max()) > 0.0
            self.G[g] = [np.array(x, np.float32) for x in out["rows"][g]]

    def op_step(self, which, h):
        lr, max_norm, eps = hyper(h)
        coef = np.asarray(self.subject.step(which, lr, max_norm, eps), np.float32)
        assert coef.shape == (self.P, 8)
        for g in range(self.P):
            row = coef[g]
            if which is not None and g not in which:
                assert bits(row, self.coef[g]), f"step: the coef row of member {g}, which sat out, changed"
                continue
            ga, gc = self.G[g]
            self.coef[g] = row.copy()
            if not (np.isfinite(ga).all() and np.isfinite(gc).all()):      # skipped whole and flagged: nothing else changes
                assert not np.isfinite(row[0]) and row[4] == 1.0 and not row[1:4].any() and not row[5:].any(), f"step: member {g} not flagged: {row}"
                continue
            want = A.coef64(ga, gc, self.step[g], lr, B1, B2, max_norm)
            for i, name in enumerate(("total_norm", "clip_coef", "step_size", "inv_sqrt_bc2")):
                assert A.within_ulps(row[i], want[i]), f"step: member {g}: {name} {float(row[i])!r}, the double expression gives {want[i]!r}"
            assert not row[4:].any(), f"step: member {g}: coef[4:] = {row[4:]}"
            new = []
            for k in (0, 1):
                p, m, v = A.step32(self.mod[g][k], self.m[g][k], self.v[g][k], self.G[g][k], row, B1, B2, eps)
                self.mod[g][k], self.m[g][k], self.v[g][k] = p, m, v
                new.append(p)
            self.set_blk(g, new)
            self.step[g] += 1

    # ---- changers
    def op_push(self):
        self.subject.push()
        for g in range(self.P):
            self.set_blk(g, self.mod[g])

    def op_push_member(self, g):
        self.subject.push_member(g)
        self.set_blk(g, self.mod[g])

    def fresh_weights(self, g, seed):
        return [perturbed(x, seed, 0.3) for x in self.init[g]]

    def op_replace_member(self, g, seed):
        new = self.fresh_weights(g, seed)
        self.subject.replace_member(g, *new)
        self.mod[g] = [x.copy() for x in new]
        self.set_blk(g, new)

    def op_replace_all(self, seeds):
        new = [None if s is None else self.fresh_weights(g, s) for g, s in enumerate(seeds)]
        self.subject.replace_all(new)
        for g in range(self.P):
            if new[g] is not None:
                self.mod[g] = [x.copy() for x in new[g]]
            self.set_blk(g, self.mod[g])                    # update_weights() of all members pushes every member

    def op_edit_in_place(self, g, how, seed):
        new = [x.copy() for x in self.mod[g]]
        if how == "load":
            ks = list(range(len(layout(self.profile))))
        else:
            ks = sorted(int(k) for k in np.random.default_rng([seed, 1]).choice(len(layout(self.profile)), size=2, replace=False))
        for k in ks:
            dst = piece(self.profile, new, k)
            dst[...] = perturbed(dst, seed + k, 0.01)
        self.subject.edit(g, how, new[0], new[1], ks)
        self.mod[g] = new

    def op_reset_opt(self, g):
        self.subject.reset_opt(g)
        for j in range(self.P) if g is None else [g]:
            self.m[j], self.v[j], self.step[j] = [np.zeros_like(x) for x in self.m[j]], [np.zeros_like(x) for x in self.v[j]], 0

    def op_move_off(self):
        self.subject.move_off()

    def op_move_on(self):
        self.subject.move_on()

    def op_rebind(self, g, k, kind, edit_seed):
        values = None
        if edit_seed is not None:
            values = perturbed(piece(self.profile, self.mod[g], k), edit_seed, 0.01)
            piece(self.profile, self.mod[g], k)[...] = values
        self.subject.rebind(g, k, kind, values)

    def op_poison(self, g, net, seed):
        j = int(np.random.default_rng([seed, 2]).integers(self.G[g][net].size))
        self.subject.poison(g, net, j)
        self.G[g][net][j] = np.float32("nan")

    def op_checkpoint(self):
        self.subject.checkpoint()
        self.ckpt = [[x.copy() for x in pair] for pair in self.mod]

    def op_load_checkpoint(self, g):
        act, val = self.subject.load_checkpoint(g)
        then = self.subject.alone(*self.ckpt[g])
        try:
            a, v = then.forward(g)
        finally:
            then.close()
        assert bits(act, a) and bits(val, v), f"load_checkpoint: a fresh policy of member {g}'s checkpoint does not compute what its weights then did"
        self.mod[g] = [x.copy() for x in self.ckpt[g]]

    def do(self, op):
        getattr(self, "op_" + op[0])(*op[1:])
        self.st.apply(op)
        self.check_all()


def run(ops, subject, upto=None, *, profile, seed):
    """Execute ``ops[:upto]`` on the subject and on the model, and compare after every op (module docstring).  A failure names the
    profile, the seed and the op index."""
    ops = list(ops if upto is None else ops[:upto])
    r = _Run(profile, seed, subject)
    i = -1
    try:
        r.check_all()
        for i, op in enumerate(ops):
            r.do(op)
    except AssertionError as e:
        listing = "\n".join(f"  {j:2d}: {o!r}" for j, o in enumerate(ops[:i + 1]))
        what = f"op {i} {ops[i]!r}" if i >= 0 else "the start"
        raise AssertionError(f"RDV_LEARNER_SEQ={profile}:{seed}:{i + 1} fails at {what}; the program up to it:\n{listing}\n{e}") from None
    finally:
        r.close()
    return r


# ------------------------------------------------------------------------------------------------------------- the real subject
class _Alone:
    """A stand-alone MlpPolicy of given weights: its handles' blocks, its forward on a member's rows, its ppo_grad"""

    def __init__(self, subject, actor, critic):
        self.s, self.policy = subject, subject.policy(actor, critic)

    def blocks(self):
        self.s.torch.cuda.synchronize()
        return tuple(A.read_block(h, 0) for h in (self.policy._hip_handle(self.s.dev), self.policy._critic_handle(self.s.dev)))

    def forward(self, g):
        obs = self.s.obs[slices(self.s.profile)[g]].contiguous()
        return self.policy.act(obs, deterministic=True).cpu().numpy(), self.policy.value(obs).cpu().numpy()

    def grads(self, g, idx):
        from reinforcement_learning_rendezvous_amd import ppo
        torch = self.s.torch
        sc = self.policy.ppo_grad(self.s.buf, torch.from_numpy(idx).to(self.s.dev), **COEFS)
        st = self.policy._ppo[self.s.dev]
        return st["actor"].cpu().numpy(), st["critic"].cpu().numpy(), torch.stack([sc[k] for k in ppo.SCALAR_NAMES]).cpu().numpy()

    def close(self):
        self.policy.close()


class SetSubject:
    """A real PolicySet on the GPU behind the methods the runner calls: modules on the CPU at first (the first device step moves them),
    both handles made by the one ``collect`` at the start, whose buffer every ``grads`` reads."""

    def __init__(self, profile, seed=11, device="cuda:0"):
        import torch
        from helpers import gpu_batch
        from reinforcement_learning_rendezvous_amd.policy import PolicySet
        self.torch, self.profile, self.dev = torch, profile, torch.device(device)
        p = PROFILES[profile]
        self.P, self.lay = len(p["sizes"]), layout(profile)
        self.pset = PolicySet([self.policy(*pair) for pair in initial(profile)], list(p["sizes"]))
        self.env = gpu_batch(sum(p["sizes"]), seed=seed)
        self.env.reset()
        self.buf = self.env.collect(self.pset, T)
        self.obs = torch.from_numpy(fixed_obs(profile)).to(self.dev)
        self.std_at = A.BLOCK_STD if self.pset.shipped_arch and list(p["vf"]) == [64, 64] else A.MLP_STD
        self.last, self.saved = None, None

    def policy(self, actor, critic):
        from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
        return MlpPolicy(weights_of(self.profile, (actor, critic)), activation_fn=PROFILES[self.profile]["act"])

    def close(self):
        self.pset.close()
        self.env.close()

    # ---- what the runner reads
    def param(self, g, k):
        """(owner, attribute) of parameter k of member g"""
        owner, _, attr = self.lay[k][0].rpartition(".")
        return (getattr(self.pset[g], owner) if owner else self.pset[g]), attr

    def flat_pair(self, tensors):
        out = [[], []]
        for (_, net, _, _), t in zip(self.lay, tensors):
            out[net].append(t.detach().reshape(-1).cpu().numpy())
        return tuple(np.concatenate(x).astype(np.float32, copy=False) for x in out)

    def state(self, g):
        sd = self.pset[g].state_dict()
        assert set(sd) == {e[0] for e in self.lay}
        return self.flat_pair([sd[e[0]] for e in self.lay])

    def blocks(self, g):
        self.torch.cuda.synchronize()
        return tuple(A.read_block(h, g) for h in (self.pset._hip_handle(self.dev), self.pset._critic_handle(self.dev)))

    def block_mismatch(self, got, want, actor):
        return A.blocks_equal(got, want, actor, self.std_at)

    def optimizer(self):
        ad = self.pset.__dict__.get("_adam", {}).get(self.dev)
        if ad is None:
            return None
        host = {k: ad[k].cpu().numpy() for k in ("actor_m", "critic_m", "actor_v", "critic_v", "step")}
        return dict(m=[(host["actor_m"][g], host["critic_m"][g]) for g in range(self.P)],
                    v=[(host["actor_v"][g], host["critic_v"][g]) for g in range(self.P)], step=host["step"])

    def alone(self, actor, critic):
        return _Alone(self, actor, critic)

    # ---- consumers
    def forward(self):
        return self.pset.act(self.obs, deterministic=True).cpu().numpy(), self.pset.value(self.obs).cpu().numpy()

    def grads(self, idx):
        from reinforcement_learning_rendezvous_amd import ppo
        torch = self.torch
        self.last = self.pset.ppo_grads(self.buf, [None if i is None else torch.from_numpy(i).to(self.dev) for i in idx], **COEFS)
        st = self.pset._ppo[self.dev]
        ra, rc = st["actor"].cpu().numpy(), st["critic"].cpu().numpy()
        out = dict(rows=[(ra[g], rc[g]) for g in range(self.P)], grad=[None] * self.P, scalars=[None] * self.P)
        for g in range(self.P):
            if self.last[g] is not None:
                out["grad"][g] = self.flat_pair([getattr(*self.param(g, k)).grad for k in range(len(self.lay))])
                out["scalars"][g] = torch.stack([self.last[g][k] for k in ppo.SCALAR_NAMES]).cpu().numpy()
        return out

    def step(self, which, lr, max_norm, eps):
        from reinforcement_learning_rendezvous_amd import ppo
        if which is not None:
            assert tuple(g for g in range(self.P) if self.last[g] is not None) == tuple(which)
        assert ppo._adam_device(self.pset) == self.dev, "the step would not take the device route"
        res = self.pset.adam_step(None if which is None else self.last, lr=lr, betas=(B1, B2), eps=eps, max_grad_norm=max_norm)
        coef = self.pset._adam[self.dev]["coef"].cpu().numpy()
        for name, col in (("total_norm", 0), ("clip_coef", 1), ("skipped", 4)):
            assert bits(res[name].cpu().numpy(), coef[:, col]), name
        return coef

    # ---- changers
    def push(self):
        self.pset.update_weights()

    def push_member(self, g):
        self.pset.update_weights(member=g)

    def replace_member(self, g, actor, critic):
        self.pset.update_weights(member=g, weights=weights_of(self.profile, (actor, critic)))

    def replace_all(self, new):
        self.pset.update_weights(weights=[None if pair is None else weights_of(self.profile, pair) for pair in new])

    def edit(self, g, how, actor, critic, ks):
        torch = self.torch
        if how == "load":
            self.pset[g].load_state_dict({e[0]: torch.from_numpy(piece(self.profile, (actor, critic), k).copy()) for k, e in enumerate(self.lay)})
        else:
            with torch.no_grad():
                for k in ks:
                    getattr(*self.param(g, k)).copy_(torch.from_numpy(piece(self.profile, (actor, critic), k).copy()))

    def reset_opt(self, g):
        self.pset.reset_optimizer(g)

    def move_off(self):
        self.pset.to("cpu")

    def move_on(self):
        self.pset.to(self.dev)

    def rebind(self, g, k, kind, values):
        torch = self.torch
        owner, attr = self.param(g, k)
        p = getattr(owner, attr)
        new = p.detach().clone()
        if values is not None:
            new.copy_(torch.from_numpy(values))
        if kind == "data":
            p.data = new
        else:
            setattr(owner, attr, torch.nn.Parameter(new, requires_grad=False))

    def poison(self, g, net, j):
        self.pset._ppo[self.dev]["actor" if net == 0 else "critic"][g, j] = float("nan")

    def checkpoint(self):
        self.saved = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.pset]

    def load_checkpoint(self, g):
        fresh = self.policy(*initial(self.profile)[0])
        try:
            fresh.load_state_dict(self.saved[g])
            obs = self.obs[slices(self.profile)[g]].contiguous()
            out = fresh.act(obs, deterministic=True).cpu().numpy(), fresh.value(obs).cpu().numpy()
        finally:
            fresh.close()
        self.pset[g].load_state_dict(self.saved[g])
        return out

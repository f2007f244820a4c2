"""
References of rdv_ppo_set_adam_step (include/rdv.h, "Gradient clip, Adam and weight repack for policy sets"; csrc/rdv_ppo_adam.h):

  - ``step32``: a NumPy float32 restatement of the elementwise step, given the four ``coef`` floats a call stores — every operation a
    float32 NumPy operation, hence rounded on its own; what the device must reproduce bit for bit;
  - ``coef64`` / ``coef32``: the double expressions of total_norm, clip_coef, step_size and inv_sqrt_bc2, and their float roundings;
  - ``step64``: the whole step in float64 — clip_grad_norm_ over actor and critic together, then torch.optim.Adam's update — and
    ``bound``, the error a float32 step may show against it, derived by counting roundings;
  - the flat layouts [5708] / [5377] of a network, the corner members that reach the packer's branches, and what the GPU tests of both
    entry points (the shipped call and rdv_ppo_mlp_set_adam_step) and the timing tools share: the gradient cases, dense gradients of any
    pair of lengths, the block reader and the block comparison.

The bound.  One step moves p by dp = step_size m / (sqrt(v) inv_sqrt_bc2 + eps).  In float32, with u = 2^-24:
  g' = g clip_coef carries 4 u (total_norm, clip_coef rounded once each from double, the product, and the gradient's own scale is exact);
  m <- m + (g' - m)(1 - beta1): the difference, the product with the float-rounded 1 - beta1 and the sum round once each.  The first two
     are relative to (1 - beta1)(|g'| + |m_old|), NOT to |m_new| (the two terms may cancel), the last to |m_new|: with g's 4 u,
     err(m) <= u (|m_new| + 7 (1 - beta1)(|g'| + |m_old|)) <= 7 u S,  S = |m_new| + (1 - beta1)(|g'| + |m_old|);
  v <- v beta2 + ((1 - beta2) g') g': two float-rounded constants, three products, one sum, g' twice: 14 u relative, halved by the root;
  the root, inv_sqrt_bc2 (rounded once) and its product, + eps (eps rounded once), the quotient, step_size (rounded once) and its product:
     8 u more.  So err(dp) <= (step_size / den) (7 u S) + 15 u |dp| <= 22 u D with D = step_size S / den >= |dp|
     (for an entry without cancellation in m, D is |dp| times 1 + (1 - beta1)(|g'| + |m_old|) / |m_new|, a number near 1 .. 2).
  p <- p - dp rounds once more: half an ulp of p.
Moments carried from earlier steps bring their own 7 u S and 7 u v of those steps, scaled down by beta1 and beta2; taking D as the largest D
of the steps so far and the constant as 32 instead of 22 covers them for the three steps the tests take.  Per step and entry:

    bound = ulp(p_new) / 2 + 32 * 2^-24 * D          (summed over the steps taken)

Nothing in it is fitted: tests/test_ppo_adam.py shows that it holds for the restatement and that four wrong restatements exceed it.
"""
import math

import numpy as np

import policy_mlp_reference as M

ACTOR, CRITIC = 5708, 5377
BLOCK_FLOATS, BLOCK_STD = 8372, 8352          # kPolFloats, kPolStd of csrc/rdv_policy.h
MLP_STD = 48                                  # kMlpStd of csrc/rdv_policy_mlp.h: exp(log_std) [8], then log_std [8], as from kPolStd on
U = 2.0 ** -24
WRONG = ("eps_in_sqrt", "no_bias_correction", "actor_norm_only", "unclamped_clip")
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------ layouts
def flat(net):
    """A policy_mlp_reference network of any depth in the flat layout of rdv_ppo_mlp_grad_floats (the shipped one: RdvPpoOut's
    w1 b1 w2 b2 w3 b3 [log_std]): per layer w then b, an actor's log_std (6 head rows) last."""
    parts = [a.reshape(-1) for w, b in zip(net["w"], net["b"]) for a in (w, b)]
    if net["w"][-1].shape[0] == 6:
        parts.append(net["log_std"].reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def unflat(vec, actor):
    """The inverse of ``flat``."""
    out = 6 if actor else 1
    vec = np.asarray(vec, np.float32)
    assert vec.shape == (ACTOR if actor else CRITIC,)
    shapes, at, ws, bs = [(64, 17), (64, 64), (out, 64)], 0, [], []
    for r, c in shapes:
        ws.append(vec[at:at + r * c].reshape(r, c).copy()); at += r * c
        bs.append(vec[at:at + r].copy()); at += r
    return M.make_net(ws, bs, "tanh", vec[at:at + 6].copy() if actor else None)


# ------------------------------------------------------------------------------------------------------------ coefficients
def coef64(ga, gc, step_before, lr, b1, b2, max_norm, wrong=None):
    """The double expressions: (total_norm, clip_coef, step_size, inv_sqrt_bc2) for a member with gradients ga [5708], gc [5377] that has
    taken ``step_before`` steps.  total_norm: math.fsum of the squares, the root in double."""
    g = [float(x) for x in ga] + ([] if wrong == "actor_norm_only" else [float(x) for x in gc])
    total = math.sqrt(math.fsum(x * x for x in g))
    t = step_before + 1
    clip = float(f32(max_norm)) / (float(f32(total)) + float(f32(1e-6)))
    if wrong != "unclamped_clip":
        clip = min(1.0, clip)
    bc1, bc2 = (1.0, 1.0) if wrong == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    return total, clip, lr / bc1, 1.0 / math.sqrt(bc2)


def coef32(*args, **kw):
    """coef64 rounded to float once each: what a call stores in coef[g][0:4], to within 1 ulp."""
    return tuple(f32(x) for x in coef64(*args, **kw))


def ulp(x):
    """The spacing of float32 at |x| (of the smallest normal below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), f32(2.0 ** -126))).astype(np.float64)


def within_ulps(got, want, n=1):
    """|got - want| <= n float32 ulps of want (want: a double expression)"""
    return abs(float(got) - want) <= n * float(ulp(f32(want)))


# ------------------------------------------------------------------------------------------------------------ the float32 restatement
def step32(p, m, v, g, coef, b1, b2, eps, wrong=None):
    """One elementwise step in float32, every operation rounded on its own: (p, m, v) <- given the four stored floats coef =
    (total_norm, clip_coef, step_size, inv_sqrt_bc2).  beta1, beta2, 1 - beta1, 1 - beta2 (differences in double) and eps are rounded to
    float once, as the host does."""
    p, m, v, g = (np.asarray(a, np.float32) for a in (p, m, v, g))
    clip, step_size, isb2 = f32(coef[1]), f32(coef[2]), f32(coef[3])
    fb2, omb1, omb2, feps = f32(b2), f32(1.0 - b1), f32(1.0 - b2), f32(eps)
    with np.errstate(all="ignore"):
        gp = g * clip
        m = m + (gp - m) * omb1
        v = v * fb2 + (omb2 * gp) * gp
        if wrong == "eps_in_sqrt":
            den = np.sqrt(v * (isb2 * isb2) + feps)
        else:
            den = np.sqrt(v) * isb2 + feps
        p = p - step_size * (m / den)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


# ------------------------------------------------------------------------------------------------------------ the float64 reference
def step64(pa, pc, ma, mc, va, vc, ga, gc, step_before, lr, b1, b2, eps, max_norm):
    """The whole step of one member in float64: clip_grad_norm_ over actor and critic together (PyTorch's clip_coef, clamped at 1, the
    1e-6 included), then torch.optim.Adam's update (no AMSGrad, no weight decay).  Arrays in, new arrays out:
    (pa, pc, ma, mc, va, vc, D) with D the scale of ``bound`` per entry, (Da, Dc)."""
    arrs = [np.asarray(a, np.float64) for a in (pa, pc, ma, mc, va, vc, ga, gc)]
    pa, pc, ma, mc, va, vc, ga, gc = arrs
    total = math.sqrt(float((ga * ga).sum() + (gc * gc).sum()))
    clip = min(1.0, max_norm / (total + 1e-6))
    t = step_before + 1
    step_size, bc2 = lr / (1.0 - b1 ** t), 1.0 - b2 ** t
    out, scale = [], []
    for p, m, v, g in ((pa, ma, va, ga), (pc, mc, vc, gc)):
        gp = g * clip
        mn = m + (gp - m) * (1.0 - b1)
        vn = v * b2 + (1.0 - b2) * gp * gp
        den = np.sqrt(vn) / math.sqrt(bc2) + eps
        out.append((p - step_size * mn / den, mn, vn))
        scale.append(step_size * (np.abs(mn) + (1.0 - b1) * (np.abs(gp) + np.abs(m))) / den)
    (pa, ma, va), (pc, mc, vc) = out
    return pa, pc, ma, mc, va, vc, tuple(scale)


def bound(p_new, d_max):
    """What one float32 step may add to |p32 - p64| per entry (the module docstring): ulp(p_new) / 2 + 32 * 2^-24 * D."""
    return 0.5 * ulp(p_new) + 32.0 * U * np.asarray(d_max, np.float64)


class Reference64:
    """A member's float64 optimiser: ``step(ga, gc)`` takes one step and grows ``tol`` (actor, critic), the summed bound."""

    def __init__(self, pa, pc, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_norm=0.5):
        self.p = [np.asarray(pa, np.float64).copy(), np.asarray(pc, np.float64).copy()]
        self.m = [np.zeros(ACTOR), np.zeros(CRITIC)]
        self.v = [np.zeros(ACTOR), np.zeros(CRITIC)]
        self.tol = [np.zeros(ACTOR), np.zeros(CRITIC)]
        self.dmax = [np.zeros(ACTOR), np.zeros(CRITIC)]
        self.steps, self.hyper = 0, (lr, betas[0], betas[1], eps, max_norm)

    def step(self, ga, gc):
        pa, pc, ma, mc, va, vc, d = step64(self.p[0], self.p[1], self.m[0], self.m[1], self.v[0], self.v[1], ga, gc, self.steps, *self.hyper)
        self.p, self.m, self.v = [pa, pc], [ma, mc], [va, vc]
        self.steps += 1
        for k in range(2):
            self.dmax[k] = np.maximum(self.dmax[k], d[k])
            self.tol[k] = self.tol[k] + bound(self.p[k], self.dmax[k])

    def worst(self, pa32, pc32):
        """max over all entries of |p32 - p64| / tol: at most 1 for a float32 step that keeps the contract"""
        return max(float((np.abs(np.asarray(x, np.float64) - p) / t).max()) for x, p, t in zip((pa32, pc32), self.p, self.tol))


# ------------------------------------------------------------------------------------------------------------ inputs
# gradient cases (name, 2-norm, max_grad_norm), in the order a test takes them as consecutive steps: the all-zero gradient first (with
# zero moments the parameters must not move), then clipping active, inactive, and no clipping at all
GRAD_CASES = [("zero", 0.0, 0.5), ("clipped", 3.0, 0.5), ("unclipped", 0.2, 0.5), ("no_clipping", 5.0, float("inf"))]


def gradients(seed, scale, ga=ACTOR, gc=CRITIC):
    """(actor, critic): dense float32 gradients of 2-norm ``scale`` over the ga + gc entries together (a gradient has no structure the
    step reads); ``scale`` 0: all zeros."""
    if scale == 0.0:
        return np.zeros(ga, np.float32), np.zeros(gc, np.float32)
    rng = np.random.default_rng([seed, 411])
    g = rng.standard_normal(ga + gc) * np.exp(rng.uniform(-2.0, 2.0, size=ga + gc))
    g = (g * (scale / np.linalg.norm(g))).astype(np.float32)
    return g[:ga].copy(), g[ga:].copy()


def corner_nets(which, seed=5):
    """(actor, critic) that reach a corner of the packer during a step of about lr = 3e-4 per entry (the critic gets the same corner):
      "cross"   one weight of layer 2 is 32 - 1e-4: the layer's max |w| crosses 2^5 if the step pushes it up, and the shift changes;
      "big"     layer 1 holds a weight of 40 (shift 9) and layer 2 one of 3000 (shift 3);
      "tiny"    layer 1's weights are about 2^-20: the lo terms are fp16-subnormal or zero;
      "zero"    an all-zero head (weights and biases: shift 10, zero fragments) and a negative-zero weight in layer 1."""
    import ppo_reference as P
    actor, critic = P.random_nets(seed=seed)
    for net in (actor, critic):
        w = [x.copy() for x in net["w"]]
        if which == "cross":
            w[1][3, 7] = f32(32.0 - 1e-4)
        elif which == "big":
            w[0][5, 2], w[1][60, 63] = f32(40.0), f32(-3000.0)
        elif which == "tiny":
            w[0] = (w[0] * f32(2.0 ** -19)).astype(np.float32)
        elif which == "zero":
            w[2] = np.zeros_like(w[2]); net["b"][2] = np.zeros_like(net["b"][2])
            w[0][0, 0] = f32(-0.0)
        else:
            raise KeyError(which)
        net["w"] = w
    return actor, critic


CORNERS = ("cross", "big", "tiny", "zero")


def read_block(handle, member, stream=None):
    """Block ``member`` of a policy handle (rdv_policy_block_floats, rdv_policy_get_block) as a float32 array"""
    import ctypes as C
    from reinforcement_learning_rendezvous_amd import _native as N
    out = np.empty(int(N.lib().rdv_policy_block_floats(handle)), np.float32)
    N.check(N.lib().rdv_policy_get_block(handle, member, out.ctypes.data_as(C.c_void_p), out.size, stream))
    return out


def blocks_equal(got, want, actor, std_at=BLOCK_STD):
    """Two parameter blocks (float32 arrays; ``std_at``: the float index of exp(log_std), BLOCK_STD in a shipped block, MLP_STD in one of
    pack_mlp_weights) compared as the header states: byte for byte outside the six exp(log_std) floats of an actor block; those within
    1 ulp of np.exp in float64 of the block's own log_std.  Returns a message, or None when equal."""
    got = np.asarray(got, np.float32)
    a, b = got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)
    assert a.shape == b.shape and (std_at != BLOCK_STD or a.shape == (BLOCK_FLOATS,))
    same = a == b
    if actor:
        same[std_at:std_at + 6] = True
    if not same.all():
        at = np.flatnonzero(~same)
        return f"{at.size} words differ, first at float {int(at[0])}: {a[at[0]]:#010x} != {b[at[0]]:#010x}"
    if actor:
        std, log_std = got[std_at:std_at + 6], got[std_at + 8:std_at + 14]
        want64 = np.exp(log_std.astype(np.float64))
        if not (np.abs(std.astype(np.float64) - want64) <= ulp(want64.astype(np.float32))).all():
            return f"exp(log_std) {std} is not within 1 ulp of {want64}"
    return None

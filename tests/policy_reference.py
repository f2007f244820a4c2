"""
NumPy reference of the policy kernels (csrc/rdv_policy.h): the 17-64-64-out tanh network in float64 and in plain float32,
Philox4x32-10 and the exploration noise restated from the contract in include/rdv.h (not from the C++), the network classes
and input sets of tests/test_gpu_policy_reference.py, and the error budget those tests assert.  Runs on the CPU; pinned by
tests/test_policy_reference.py.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IN, HID, OUT = 17, 64, 6
OBS_CLAMP = 63.0                 # rdv.h: observations are clamped to +-63 before the network (NaN stays NaN)
TANH_ABS_ERR = 2.5e-7            # rdv_policy.h: documented absolute error of the kernel's tanh
SUBNORMAL_ABS_ERR = 6e-8         # rdv_policy.h: documented absolute loss of an input below 1.2e-4 (fp16 subnormal lo term)
# Tolerance on a standard normal of the kernel's fp32 Box-Muller (__logf, __sincosf: no ULP bound is documented for gfx950)
# against actor_normals: 4 x the maximum measured by test_gpu_policy_reference.test_fast_normals_against_fp64 over 25 million
# normals, 2.4414e-4.  That maximum is not an intrinsic's error: for the top word (w >> 8 = 2^24 - 1) the fp32 sum (w >> 8) + 0.5
# rounds to 2^24, u1 becomes exactly 1 and the kernel's pair is (0, 0) where the exact radius is sqrt(2^-24) = 2^-12 — the largest
# such loss there is (any w >> 8 >= 2^23 loses its half).  Over the pairs with u1 < 1 - 2^-20 the same run measured 1.91e-5.
TOL_Z = 9.77e-4
ACTOR_KEYS = ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
              "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias"]
CRITIC_KEYS = ["mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
               "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias"]


# ------------------------------------------------------------------------------------------------------------ the network
def make_net(w1, b1, w2, b2, w3, b3, log_std=None):
    """A network as a dict of float32 arrays (SB3 layout, nn.Linear [out, in])."""
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    net = dict(w1=f(w1), b1=f(b1), w2=f(w2), b2=f(b2), w3=f(w3), b3=f(b3))
    net["log_std"] = f(np.zeros(net["w3"].shape[0]) if log_std is None else log_std)
    assert net["w1"].shape == (HID, IN) and net["w2"].shape == (HID, HID) and net["w3"].shape[1] == HID
    return net


def critic_of(net):
    """The out_dim = 1 network that shares a class's trunk: its first head row."""
    return make_net(net["w1"], net["b1"], net["w2"], net["b2"], net["w3"][:1], net["b3"][:1])


def clamp_obs(obs):
    return np.clip(obs, -OBS_CLAMP, OBS_CLAMP)        # np.clip keeps NaN


def _mlp(net, obs, dt):
    x = np.asarray(obs, dtype=np.float32).astype(dt)  # float32 -> float64 is exact
    p = {k: net[k].astype(dt) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    h1 = np.tanh(x @ p["w1"].T + p["b1"])
    h2 = np.tanh(h1 @ p["w2"].T + p["b2"])
    y = h2 @ p["w3"].T + p["b3"]
    assert y.dtype == dt
    return y


def mlp64(net, obs):
    """W3 tanh(W2 tanh(W1 obs + b1) + b2) + b3 in float64 from the float32 parameters; no clipping of inputs or outputs."""
    return _mlp(net, obs, np.float64)


def mlp32(net, obs):
    """The same in plain NumPy float32: the 'ordinary fp32 evaluation' yardstick."""
    return _mlp(net, obs, np.float32)


def error_floor(net):
    """A = |W3|inf (d + |W2|inf (d + |W1|inf 6e-8)), d = TANH_ABS_ERR: what the kernel does not share with a correctly rounded fp32
    evaluation (its tanh's absolute error and the loss of subnormal lo terms of tiny inputs), propagated through the network
    with tanh' <= 1.  |.|inf is the largest absolute row sum."""
    n = lambda w: float(np.abs(w.astype(np.float64)).sum(axis=1).max())
    return n(net["w3"]) * (TANH_ABS_ERR + n(net["w2"]) * (TANH_ABS_ERR + n(net["w1"]) * SUBNORMAL_ABS_ERR))


def error_floor_entrywise(net):
    """The same two constants propagated entry by entry instead of by norms: max_c (|W3| (d 1 + |W2| (d 1 + |W1| 6e-8 1)))_c.
    Never above error_floor (|M| v <= |M|inf max v); much below it when a network's large weights do not chain, as in
    shift_lt_10, whose norm product is useless (A ~ 10)."""
    a = lambda k: np.abs(net[k].astype(np.float64))
    e1 = a("w1") @ np.full(IN, SUBNORMAL_ABS_ERR)
    e2 = a("w2") @ (e1 + TANH_ABS_ERR)
    return float((a("w3") @ (e2 + TANH_ABS_ERR)).max())


def documented_shift(w):
    """rdv.h: a layer's weights enter the matrix cores times 2^s, s the largest integer <= 10 with max|w| 2^s < 2^15."""
    mx = float(np.abs(w).max())
    s = 10
    while s > -20 and mx * 2.0 ** s >= 2.0 ** 15:
        s -= 1
    return s


# ------------------------------------------------------------------------------------------------------------------ noise
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011).  counter: four words, key: two words, each an integer or an integer array (broadcast
    against each other); returns uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _M32 for x in key)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0 = np.uint64(0xD2511F53) * c[0]             # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


POLICY_KEY_TWEAK = 0x504F4C49


def actor_words(seed, env_ids, counter):
    """The two Philox blocks of each env: uint32 [n, 2, 4].  Block h has counter words (id_lo, id_hi, counter_lo,
    counter_hi * 2 + h) and key (seed_lo, seed_hi ^ 0x504F4C49)."""
    ids = np.asarray(env_ids, dtype=np.uint64).reshape(-1)
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, (seed >> 32) ^ POLICY_KEY_TWEAK)
    blocks = [philox4x32_10((ids & _M32, ids >> _S32, counter & 0xFFFFFFFF, ((counter >> 32) * 2 + h) & 0xFFFFFFFF), key)
              for h in (0, 1)]
    return np.stack(blocks, axis=1)


def uniforms(words):
    return ((words >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0


def actor_normals(seed, env_ids, counter, return_uniforms=False):
    """Standard normals [n, 6] (float64) of the exploration noise of action components 0..5 of the given GLOBAL env ids at call
    `counter`: block 0 -> components 0..3, block 1 -> components 4, 5; per word pair (0,1) and (2,3):
    u = ((w >> 8) + 0.5) / 2^24, (z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2)."""
    u = uniforms(actor_words(seed, env_ids, counter))                        # [n, 2, 4]
    u1, u2 = u[:, :, 0::2], u[:, :, 1::2]                                     # [n, block, pair]
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1)   # [n, block, pair, (cos, sin)]
    z = z.reshape(len(u), 8)[:, :6]                                           # block 0: 4 normals, block 1: its first pair
    if return_uniforms:
        return z, u1.reshape(len(u), 4)[:, :3], u2.reshape(len(u), 4)[:, :3]
    return z


def log_prob64(z, log_std):
    return (-0.5 * z * z - np.asarray(log_std, np.float64)).sum(axis=1) - 3.0 * np.log(2.0 * np.pi)


# ------------------------------------------------------------------------------------------------------- network classes
def shipped(critic=False):
    g = np.load(os.path.join(GOLDEN, "mlp_policy.npz"), allow_pickle=False)
    if critic:
        return make_net(*[g[k] for k in CRITIC_KEYS])
    return make_net(*[g[k] for k in ACTOR_KEYS], log_std=g["log_std"])


def _dense(rng, s1=0.35, s2=0.18, s3=0.08, sb=0.1):
    return [rng.normal(scale=s1, size=(HID, IN)), rng.normal(scale=sb, size=HID), rng.normal(scale=s2, size=(HID, HID)),
            rng.normal(scale=sb, size=HID), rng.normal(scale=s3, size=(OUT, HID)), rng.normal(scale=sb, size=OUT)]


def fresh_init(seed=11):
    """What a training run starts from: MlpPolicy(weights=None): orthogonal, gains sqrt 2, sqrt 2, 0.01, zero biases."""
    from helpers import to_numpy as a
    from reinforcement_learning_rendezvous_amd.policy import MlpPolicy
    p = MlpPolicy(weights=None, seed=seed)
    return make_net(a(p.l1.weight), a(p.l1.bias), a(p.l2.weight), a(p.l2.bias), a(p.l3.weight), a(p.l3.bias))


def shift_lt_10(seed=12):
    """A moderate dense network with a few outlier weights per layer, so that max|w| lands in [32,64), [256,512), [4096,8192):
    shifts 9, 6, 2.  Layer-1 outliers saturate their own hidden unit only; the layer-2 and head outliers read hidden units
    that are kept small (tiny incoming weights, zero bias), so their products stay O(0.1)."""
    rng = np.random.default_rng(seed)
    w1, b1, w2, b2, w3, b3 = _dense(rng)
    quiet1, quiet2 = [5, 38, 61], [9, 30, 52]          # hidden units of layer 1 / layer 2 that are kept small
    w1[quiet1] *= 2.0 ** -9; b1[quiet1] = 0.0
    w2[quiet2] *= 2.0 ** -13; b2[quiet2] = 0.0
    w2[:, quiet1] *= 0.0
    for (p, k), v in zip([(3, 2), (40, 16), (57, 9)], (41.5, -35.25, 55.0)):
        w1[p, k] = v
    for (p, k), v in zip([(7, 5), (33, 38), (60, 61)], (300.0, -410.5, 270.0)):
        w2[p, k] = v
    w3[:, quiet2] = 0.0
    for (p, k), v in zip([(0, 9), (3, 30), (5, 52)], (5000.0, -6100.0, 4500.5)):
        w3[p, k] = v
    return make_net(w1, b1, w2, b2, w3, b3)


def tiny(seed=13):
    """A dense network with |w| < 0.5, times 2^-12 (weights and biases): scaled by 2^10 every weight is below 2^-3, so every
    lo term (<= 2^-15) is an fp16 subnormal or zero."""
    rng = np.random.default_rng(seed)
    return make_net(*[np.clip(p, -0.49, 0.49) * 2.0 ** -12 for p in _dense(rng, s1=0.25, s2=0.15, s3=0.12)])


def big_bias(seed=14):
    """Hidden biases up to +-30 on half of the units (saturated beside live ones), head biases up to +-0.9."""
    rng = np.random.default_rng(seed)
    w1, b1, w2, b2, w3, b3 = _dense(rng, s3=0.01)
    for b in (b1, b2):
        hot = rng.permutation(HID)[:HID // 2]
        b[hot] = rng.uniform(-30.0, 30.0, size=hot.size)
    b1[0], b2[63] = 30.0, -30.0
    b3 = rng.uniform(-0.9, 0.9, size=OUT); b3[0], b3[5] = 0.9, -0.9
    return make_net(w1, b1, w2, b2, w3, b3)


ROUTE_NETS = 11                  # 11 x 6 head rows >= 64: every hidden index of both layers reaches an output


def route_probe(m, seed=15):
    """Sparse one-hot network number m (0 <= m < ROUTE_NETS).  Output c reads ONE path:
        feature[c] --1.0--> hidden-1 unit src[c] --sign 0.5--> hidden-2 unit mid[c] --0.75--> output c
    with distinct biases on every unit.  Over the ROUTE_NETS networks src and mid each cover 0..63.  Returns the network and
    the path table dict(feature, src, mid, sign) (arrays of 6)."""
    rng = np.random.default_rng(seed)
    sigma, tau = rng.permutation(HID), rng.permutation(HID)                  # the same for every m
    rng = np.random.default_rng(seed * 1000 + m)
    src = sigma[(6 * m + np.arange(OUT)) % HID]
    mid = tau[(6 * m + np.arange(OUT)) % HID]
    feature = (6 * m + np.arange(OUT)) % IN
    # input k -> hidden-1 unit p1[k]: the six probed features go to src, the others to random free units
    free = rng.permutation(np.setdiff1d(np.arange(HID), src))
    p1 = np.empty(IN, int); p1[feature] = src
    rest = np.setdiff1d(np.arange(IN), feature); p1[rest] = free[:rest.size]
    # signed permutation x 0.5 with p2[src] = mid
    p2 = np.empty(HID, int); p2[src] = mid
    others = np.setdiff1d(np.arange(HID), src)
    p2[others] = rng.permutation(np.setdiff1d(np.arange(HID), mid))
    sign = rng.choice([-1.0, 1.0], size=HID)
    w1 = np.zeros((HID, IN)); w1[p1, np.arange(IN)] = 1.0
    w2 = np.zeros((HID, HID)); w2[p2, np.arange(HID)] = 0.5 * sign
    w3 = np.zeros((OUT, HID)); w3[np.arange(OUT), mid] = 0.75
    b1 = rng.permutation(np.linspace(-0.6, 0.6, HID))
    b2 = rng.permutation(np.linspace(-0.4, 0.4, HID))
    b3 = np.linspace(-0.1, 0.1, OUT)
    return make_net(w1, b1, w2, b2, w3, b3), dict(feature=feature, src=src, mid=mid, sign=sign[src])


def route_scalar64(net, path, obs):
    """The fp64 reference of a route_probe network as a composition of three scalar tanh's per output."""
    x = clamp_obs(np.asarray(obs, np.float32)).astype(np.float64)[:, path["feature"]]
    f = lambda k: net[k].astype(np.float64)
    h1 = np.tanh(x + f("b1")[path["src"]])
    h2 = np.tanh(0.5 * path["sign"] * h1 + f("b2")[path["mid"]])
    return 0.75 * h2 + f("b3")


def with_log_std(net, log_std=(-5.0, -0.5, 0.0, 1.0, -0.5, 0.0)):
    out = dict(net); out["log_std"] = np.asarray(log_std, np.float32)
    return out


def network_classes():
    """id -> list of (network, path table or None); route_probe is a list of ROUTE_NETS networks."""
    return {"shipped": [(shipped(), None)], "fresh_init": [(fresh_init(), None)], "shift_lt_10": [(shift_lt_10(), None)],
            "tiny": [(tiny(), None)], "big_bias": [(big_bias(), None)],
            "route_probe": [route_probe(m) for m in range(ROUTE_NETS)]}


# ------------------------------------------------------------------------------------------------------------ input sets
BATCH_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 65536, 65537)


def distinct_rows(n, seed=0):
    """float32 rows, every row distinct (asserted): even rows are real observations (the golden trajectories, cycled) with a
    N(0, 0.02) jitter, odd rows U(-1,1).  (The shipped actor saturates on three quarters of U(-1,1) rows: uniform rows alone
    would leave the clip to hide its errors.)"""
    rng = np.random.default_rng(1000 + seed)
    x = rng.uniform(-1.0, 1.0, size=(n, IN))
    real = np.concatenate(list(golden_obs().values()))
    even = np.arange(0, n, 2)
    x[even] = real[rng.integers(0, len(real), size=even.size)] + rng.normal(scale=0.02, size=(even.size, IN))
    x = x.astype(np.float32)
    assert len(np.unique(np.ascontiguousarray(x[:, :2]).view(np.dtype((np.void, 8))))) == n
    return x


def magnitude_ladder(seed=1):
    """For k = 0..30: a row of +-m 2^-k (m in [1,2)), the same with five O(1) entries mixed in, and an O(1) neighbour."""
    rng = np.random.default_rng(2000 + seed)
    rows = []
    for k in range(31):
        small = rng.choice([-1.0, 1.0], size=IN) * rng.uniform(1.0, 2.0, size=IN) * 2.0 ** -k
        mixed = small.copy()
        at = rng.permutation(IN)[:5]
        mixed[at] = rng.uniform(-1.0, 1.0, size=5)
        rows += [small, mixed, rng.uniform(-1.0, 1.0, size=IN)]
    return np.asarray(rows, dtype=np.float32)


def exact_rows():
    alt = np.where(np.arange(IN) % 2 == 0, 1.0, -1.0)
    rows = [np.zeros(IN), np.ones(IN), -np.ones(IN), alt, -alt]
    for v in (1.0, -0.5):
        rows += list(v * np.eye(IN))                  # a single non-zero feature, each of the 17 in turn
    return np.asarray(rows, dtype=np.float32)


def clamp_rows(seed=2):
    """Entries at +-62.9, +-63, +-64, +-1e4, +-inf: one such entry in an O(1) row (each feature in turn), and whole rows."""
    rng = np.random.default_rng(3000 + seed)
    rows, k = [], 0
    for v in (62.9, 63.0, 64.0, 1e4, np.inf):
        for s in (1.0, -1.0):
            for _ in range(4):
                r = rng.uniform(-1.0, 1.0, size=IN); r[k % IN] = s * v; k += 5
                rows.append(r)
            rows.append(np.full(IN, s * v))
    return np.asarray(rows, dtype=np.float32)


def golden_obs():
    out = {}
    for name in ("steps_B_mc_policy.npz", "steps_D_stochastic.npz"):
        g = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        o = np.concatenate([g["obs0"].reshape(-1, IN), g["obs_ret"].reshape(-1, IN)]).astype(np.float32)
        out[name[:7]] = o[np.isfinite(o).all(axis=1)]
    return out


def input_sets():
    sets = {f"n{n}": distinct_rows(n, seed=n) for n in BATCH_SIZES}
    sets["ladder"], sets["exact"], sets["clamp"] = magnitude_ladder(), exact_rows(), clamp_rows()
    sets.update(golden_obs())
    return sets


def unsaturated_share(nets, sets):
    """Share of the fp64 action components over all input sets that lie strictly inside (-0.999, 0.999) before clipping."""
    inside = total = 0
    for net, _ in nets:
        for x in sets.values():
            y = mlp64(net, clamp_obs(x))
            inside += int((np.abs(y) < 0.999).sum()); total += y.size
    return inside / total

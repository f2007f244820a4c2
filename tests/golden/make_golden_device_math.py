"""
Regenerates tests/golden/device_math_reference*.npz (five files, FILES below): inputs of the numerical primitives of csrc/rdv_device.h
and what each of them should return, evaluated with mpmath at 50 digits from the formulas the header cites.  Nothing here reads the product or a GPU.

    python tests/golden/make_golden_device_math.py

Every expected value x is stored as a pair of doubles, hi = RN(x) and lo = RN(x - hi), so that the GPU test (tests/
test_gpu_device_math.py) measures errors far below an ulp with NumPy alone (tests/device_probe.py: ulp_error).  The inputs are built
from exact operations only (integers, ldexp, nextafter, IEEE + - * / sqrt on seeded uniform bits) — no libm call — so that every host
regenerates the same file; tests/test_device_math_reference.py asserts that.

Keys: `<set>_<input>` for the inputs, `<set>_<output>_hi` / `_lo` for the results.  Primitives whose reference is exact integer or
IEEE arithmetic (div_1e5, u21, s21, philox4x32_10, normalized) and the 200,001-entry acos table (1.6 MB of doubles: evaluated at
test time by acos_reference below) have no arrays here.
"""
import functools
import os

import mpmath
import numpy as np
from mpmath import mpf

mpmath.mp.dps = 50

HERE = os.path.dirname(os.path.abspath(__file__))
# No committed file may exceed 1 MiB and doubles do not compress, so the fixture is five files of one scheme, by set of arrays (the
# prefix of the key): the scalar functions in device_math_reference.npz, the vector ones beside it.
FILES = {"device_math_reference.npz": ("rsqrt", "rsqrtsub", "tiny", "small", "switch", "pow"),
         "device_math_reference_vectors.npz": ("large", "unit", "rms", "q2msub"),
         "device_math_reference_quat2mat.npz": ("q2m",),
         "device_math_reference_deviate.npz": ("dev", "devtiny"),
         "device_math_reference_attitude.npz": ("ia", "iaraw")}
K_TINY_U = 0.0078125          # rdv_device.h: kTinyU
K_SMALL_U = 0.62              # rdv_device.h: kSmallU
HALF_DT = 0.5                 # the default parameters' dt / 2
N_RANDOM = 4096


# ------------------------------------------------------------------------------------------------------------ encoding
def split(x):
    """mpf -> (hi, lo) = (RN(x), RN(x - hi))"""
    hi = float(x)
    return hi, float(x - mpf(hi))


def encode(values):
    """iterable of mpf (or of tuples of mpf) -> hi, lo arrays of the same shape"""
    rows = [[split(v) for v in (r if isinstance(r, (tuple, list)) else (r,))] for r in values]
    a = np.array(rows, dtype=np.float64)                # [n, m, 2]
    hi, lo = a[..., 0], a[..., 1]
    if hi.shape[1] == 1:
        hi, lo = hi[:, 0], lo[:, 0]
    return np.ascontiguousarray(hi), np.ascontiguousarray(lo)


def odd(x):
    """the array with an odd length (the last element dropped if needed): no probe launch is a whole number of 256-thread blocks"""
    return x if len(x) % 2 == 1 else x[:-1]


def neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)])


def log_uniform(rng, n, e_lo, e_hi, lo, hi):
    """n doubles m 2^e, m uniform in [1, 2), e uniform in e_lo .. e_hi, clipped to [lo, hi] (exact operations only)"""
    return np.clip(np.ldexp(1.0 + rng.random(n), rng.integers(e_lo, e_hi + 1, n).astype(np.int32)), lo, hi)


def unit_rows(rng, n, m):
    v = rng.random((n, m)) * 2.0 - 1.0
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


# ------------------------------------------------------------------------------------------------------------ inputs
def build_inputs():
    rng = np.random.default_rng(20250801)
    I = {}
    # rsqrt64: 4^k and both neighbours, random mantissas at even and at odd exponents, a sweep of [0.25, 4), the whole normal range
    pow4 = np.ldexp(1.0, (2 * np.arange(-500, 501)).astype(np.int32))
    even = np.ldexp(1.0 + rng.random(1024), (2 * rng.integers(-500, 501, 1024)).astype(np.int32))
    oddx = np.ldexp(1.0 + rng.random(1024), (2 * rng.integers(-500, 500, 1024) + 1).astype(np.int32))
    sweep = 0.25 + np.arange(1024) * (3.75 / 1024)
    whole = np.ldexp(1.0 + rng.random(N_RANDOM), rng.integers(-1022, 1023, N_RANDOM).astype(np.int32))
    I["rsqrt_x"] = odd(np.concatenate([neighbours(pow4), even, oddx, sweep, whole]))
    # subnormal arguments k 2^-1074: the smallest even and odd k, then random k up to 2^52
    k = np.concatenate([np.arange(2, 66), rng.integers(66, 1 << 52, 959)]).astype(np.float64)
    I["rsqrtsub_x"] = np.ldexp(k, np.int32(-1074))
    # cos_sinc_tiny on [0, 2^-7], cos_sinc_small on [0, 0.62]
    top = K_TINY_U
    I["tiny_u"] = odd(np.concatenate([[0.0, top, np.nextafter(top, 0.0), 5e-324, 1e-300], np.ldexp(1.0, -np.arange(8, 61).astype(np.int32)),
                                      np.arange(513) * (top / 512), rng.random(N_RANDOM) * top]))
    top = K_SMALL_U
    I["small_u"] = odd(np.concatenate([[0.0, top, np.nextafter(top, 0.0), 5e-324, K_TINY_U], np.arange(513) * (top / 512),
                                       rng.random(N_RANDOM) * top]))
    # the dispatcher: both switches, three doubles either side, one ulp apart
    def around(x):
        below = [x]
        for _ in range(3):
            below.append(np.nextafter(below[-1], 0.0))
        above = [x]
        for _ in range(3):
            above.append(np.nextafter(above[-1], np.inf))
        return below[::-1] + above[1:]
    I["switch_u"] = np.array(around(K_TINY_U) + around(K_SMALL_U) + [0.0], dtype=np.float64)
    # cos_sinc_large on (0.62, 1e6]: both sides of every halving threshold 0.62 4^h, a log-uniform sample, and some h = 0 arguments
    edges = np.array([K_SMALL_U * 4.0 ** h for h in range(0, 11)])
    I["large_u"] = odd(np.concatenate([edges[1:], np.nextafter(edges, np.inf), [1e6, np.nextafter(1e6, 0.0)],
                                       log_uniform(rng, N_RANDOM, -1, 19, np.nextafter(K_SMALL_U, 1.0), 1e6),
                                       np.nextafter(K_SMALL_U, 1.0) + np.arange(256) * ((1e6 - 1.0) / 256),
                                       K_TINY_U + rng.random(255) * (K_SMALL_U - K_TINY_U)]))
    # pow_minus_fifth: 2^e and neighbours for e = -60 .. 60 (every residue of e mod 5, both signs), either side of 1, the callers' range
    one = [1.0]
    for _ in range(16):
        one = [np.nextafter(one[0], 0.0)] + one + [np.nextafter(one[-1], 2.0)]
    I["pow_x"] = odd(np.concatenate([neighbours(np.ldexp(1.0, np.arange(-60, 61).astype(np.int32))), one,
                                     log_uniform(rng, 512, -27, 43, 1e-8, 1e13), log_uniform(rng, N_RANDOM, -27, 43, 1e-8, 1e13)]))
    # unit_vector: draws of s21 (field 2^-20 + 2^-21 - 1), the corners and the smallest components
    f = rng.integers(0, 1 << 21, (N_RANDOM, 3))
    corner = np.array([[0, 0, 0], [(1 << 21) - 1] * 3, [1 << 20] * 3, [(1 << 20) - 1] * 3, [1 << 20, (1 << 20) - 1, 1 << 20],
                       [0, 1 << 20, 1 << 20], [1 << 20, 1 << 20, 0], [(1 << 21) - 1, 1 << 20, (1 << 20) - 1], [5, 1 << 20, 77]])
    I["unit_v"] = np.concatenate([corner, f]).astype(np.float64) * (1.0 / 1048576.0) + (1.0 / 2097152.0 - 1.0)
    # quat2mat: unit, non-unit (norm 0.3 .. 13), axis-aligned; and quaternions whose squared norm is subnormal, on their own
    q = unit_rows(rng, N_RANDOM, 4)
    scaled = unit_rows(rng, 512, 4) * (0.3 + rng.random(512) * 12.7)[:, None]
    fixed = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [3.0, -4.0, 12.0, 0.5], [-1, 0, 0, 0], [0.5, 0.5, 0.5, 0.5],
                      [1e-150, 0, 0, 1e-150], [1e150, -1e150, 0, 1e150]], dtype=np.float64)
    I["q2m_q"] = np.concatenate([fixed, q, scaled])
    tiny = unit_rows(rng, 254, 4) * (1e-160 * (0.5 + rng.random(254) * 4.0))[:, None]
    I["q2msub_q"] = np.concatenate([np.array([[1e-160, 0.0, 0.0, 1e-160]]), tiny])
    # deviate: angles across [0, pi] with tiny = 0; angles up to the largest range that sets tiny = 1, with either setting
    n = N_RANDOM + 513
    theta_max_tiny = 2.0 * np.sqrt(K_TINY_U)                     # 0.25 range^2 <= kTinyU (derive_params): range <= 0.17677...
    while 0.25 * theta_max_tiny * theta_max_tiny > K_TINY_U:
        theta_max_tiny = np.nextafter(theta_max_tiny, 0.0)
    I["dev_axis"] = unit_rows(rng, n, 3)
    I["dev_nominal"] = unit_rows(rng, n, 4)
    I["dev_theta"] = np.concatenate([[0.0, np.pi, np.nextafter(np.pi, 0.0), theta_max_tiny, np.nextafter(theta_max_tiny, 1.0)],
                                     np.arange(508) * (np.pi / 508), rng.random(N_RANDOM) * np.pi])
    n = 1024 + 513
    I["devtiny_axis"] = unit_rows(rng, n, 3)
    I["devtiny_nominal"] = unit_rows(rng, n, 4)
    I["devtiny_theta"] = np.concatenate([[0.0, theta_max_tiny, np.nextafter(theta_max_tiny, 0.0), 5e-324, 1e-8],
                                         np.arange(508) * (theta_max_tiny / 508), rng.random(1024) * theta_max_tiny])
    # integrate_attitude: |w| dt/2 up to pi/2 (every cos_sinc branch, one halving at the most), w = 0 exactly
    mag = np.concatenate([[0.0, 0.0, 0.0], rng.random(1366) * 0.17, 0.18 + rng.random(1365) * 1.39, 1.58 + rng.random(1365) * 1.55,
                          np.sqrt(np.array(around(K_TINY_U) + around(K_SMALL_U))) / HALF_DT])
    I["ia_w"] = unit_rows(rng, len(mag), 3) * mag[:, None]
    I["ia_q"] = unit_rows(rng, len(mag), 4)
    # ... and the form for injected states: |q| from 1e-3 to 1e3, and |q|^2 - 1 either side of 1e-6
    mag = np.concatenate([[0.0, 0.0, 0.0], rng.random(906) * 0.17, 0.18 + rng.random(905) * 1.39, 1.58 + rng.random(905) * 1.55,
                          np.sqrt(np.array(around(K_TINY_U) + around(K_SMALL_U))) / HALF_DT])
    scale = np.ldexp(1.0 + rng.random(len(mag)), rng.integers(-10, 10, len(mag)).astype(np.int32))
    d = 1e-6 * np.array([1.001, 0.999, -1.001, -0.999, 1.01, 0.99, -1.01, -0.99])
    scale[3:3 + len(d)] = np.sqrt(1.0 + d)
    scale[20:40] = 1.0
    I["iaraw_q"] = unit_rows(rng, len(mag), 4) * scale[:, None]
    # a quaternion of norm rho turns at w / rho: the rate is scaled with rho, so that the angle the series sees, |w| dt/2 / rho, covers
    # every branch with one halving at the most, as above (what larger angles cost is cos_sinc_large's own measurement)
    rho = np.sqrt((I["iaraw_q"] * I["iaraw_q"]).sum(axis=1))
    rho[np.abs(rho * rho - 1.0) <= 1.5e-6] = 1.0
    I["iaraw_w"] = unit_rows(rng, len(mag), 3) * (mag * rho)[:, None]
    # rms7: seven values of mixed magnitude, equal values, one dominant value, zeros
    x = (rng.random((N_RANDOM, 7)) * 2.0 - 1.0) * np.ldexp(1.0, rng.integers(-10, 11, (N_RANDOM, 7)).astype(np.int32))
    fixed = np.array([[0.0] * 7, [1.0] * 7, [1e3, 0, 0, 0, 0, 0, 0], [1e-9] * 7, [3.0, -4.0, 12.0, 0.5, 1e-5, 2.5, -7.0]])
    I["rms_x"] = np.concatenate([fixed, x])
    for name, a in I.items():
        assert len(a) % 2 == 1 and len(a) <= 65536, (name, len(a))
    return I


# ------------------------------------------------------------------------------------------------------------ the formulas
def m_cos_sinc(u):
    """cos(t), sin(t)/t for t = sqrt(u)"""
    t = mpmath.sqrt(mpf(u))
    return (mpmath.cos(t), mpmath.sin(t) / t) if t != 0 else (mpf(1), mpf(1))


def m_normalize(v):
    n = mpmath.sqrt(sum(x * x for x in v))
    return [x / n for x in v]


def m_quat_product(a, b):
    """quaternions.py:149-170, scalar first"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def m_quat2mat(q):
    """quaternions.py:48-68: R of the normalised quaternion"""
    w, x, y, z = m_normalize([mpf(v) for v in q])
    return [2 * (w * w + x * x) - 1, 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 2 * (w * w + y * y) - 1, 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 2 * (w * w + z * z) - 1]


def m_deviate(axis, theta, nominal):
    """quat_product(rot2quat(axis, theta), nominal) with the reference's normalisations of the axis and of both factors; the product
    itself is not normalised (rdv_device.h: deviate)"""
    a = m_normalize([mpf(v) for v in axis])
    half = mpf(theta) / 2
    rot = m_normalize([mpmath.cos(half)] + [v * mpmath.sin(half) for v in a])
    return m_quat_product(rot, m_normalize([mpf(v) for v in nominal]))


def m_integrate_attitude(q, w, half_dt, raw):
    """normalize(q (x) [cos a, w_hat sin a]), a = |w| dt/2 / rho.  rho = 1, except in the form for injected states (raw) with
    | |q|^2 - 1 | > 1e-6, where rho = |q| (rdv_device.h: integrate_attitude)"""
    q = [mpf(v) for v in q]
    w = [mpf(v) for v in w]
    n2 = sum(v * v for v in q)
    h = mpf(half_dt)
    if raw and abs(n2 - 1) > mpf(1e-6):
        h = h / mpmath.sqrt(n2)
    wn = mpmath.sqrt(sum(v * v for v in w))
    a = wn * h
    sinc = mpmath.sin(a) / a if a != 0 else mpf(1)
    return m_normalize(m_quat_product(q, [mpmath.cos(a)] + [v * sinc * h for v in w]))


@functools.lru_cache(maxsize=1)
def acos_reference():
    """(hi, lo) of acos(k / 1e5) for k = -100000 .. 100000, k / 1e5 being the double NumPy's division gives (correctly rounded; the
    table's argument).  Not in the fixture (1.6 MB as doubles); about two seconds."""
    x = np.arange(0, 100001) / 1e5
    pi = mpmath.pi
    pos = [mpmath.acos(mpf(v)) for v in x]                 # (-k) / 1e5 = -(k / 1e5) exactly: acos(-x) = pi - acos(x)
    hi, lo = encode([pi - v for v in pos[:0:-1]] + pos)
    return hi, lo


# ------------------------------------------------------------------------------------------------------------ the fixture
def generate():
    I = build_inputs()
    G = dict(I)

    def put(name, values):
        G[name + "_hi"], G[name + "_lo"] = encode(values)

    put("rsqrt_y", [1 / mpmath.sqrt(mpf(x)) for x in I["rsqrt_x"]])
    put("rsqrtsub_y", [1 / mpmath.sqrt(mpf(x)) for x in I["rsqrtsub_x"]])
    for name in ("tiny", "small", "switch", "large"):
        cs = [m_cos_sinc(u) for u in I[name + "_u"]]
        put(name + "_c", [c for c, _ in cs])
        put(name + "_sc", [s for _, s in cs])
    put("pow_y", [mpmath.root(mpf(x), 5) ** -1 for x in I["pow_x"]])
    put("unit_o", [m_normalize([mpf(c) for c in v]) for v in I["unit_v"]])
    put("q2m_m", [m_quat2mat(q) for q in I["q2m_q"]])
    put("q2msub_m", [m_quat2mat(q) for q in I["q2msub_q"]])
    put("dev_o", [m_deviate(a, t, b) for a, t, b in zip(I["dev_axis"], I["dev_theta"], I["dev_nominal"])])
    put("devtiny_o", [m_deviate(a, t, b) for a, t, b in zip(I["devtiny_axis"], I["devtiny_theta"], I["devtiny_nominal"])])
    put("ia_o", [m_integrate_attitude(q, w, HALF_DT, False) for q, w in zip(I["ia_q"], I["ia_w"])])
    put("iaraw_o", [m_integrate_attitude(q, w, HALF_DT, True) for q, w in zip(I["iaraw_q"], I["iaraw_w"])])
    put("rms_y", [mpmath.sqrt(sum(mpf(v) * mpf(v) for v in x) / 7) for x in I["rms_x"]])
    return G


if __name__ == "__main__":
    g = generate()
    for name, sets in FILES.items():
        part = {k: v for k, v in g.items() if k.split("_")[0] in sets}
        np.savez_compressed(os.path.join(HERE, name), **part)
        print(f"wrote {name}: {len(part)} arrays, {os.path.getsize(os.path.join(HERE, name))} bytes")
    assert sum(len(s) for s in FILES.values()) == len({k.split("_")[0] for k in g})

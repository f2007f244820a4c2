"""
The numerical primitives of csrc/rdv_device.h, one by one, against a 50-digit reference (run with `-m gpu`).

The transition tests compare whole steps at 1e-10 (state), 2.4e-7 (observation) and 1e-6 (diagnostics); a primitive could be 1e-12 off
underneath them.  Here each primitive runs alone (librdv_probe.so: csrc/rdv_probe.hip, compiled with the product's flags;
tests/device_probe.py) on the inputs of tests/golden/device_math_reference*.npz and is held to the bound its comment in the header
claims, measured with device_probe.ulp_error: |(got - hi) - lo| / spacing(|hi|).  Every launch has an odd length (a ragged last
block).  Each test prints the maximum it measured (`device_math ...` lines; profiles/device_math_ulp.txt is that output).

Bounds, and where they come from (eps = 2^-53, "ulp" = spacing of doubles at the result):

  rsqrt64           2 ulp      the header's claim.  After two Newton steps from v_rsq_f64 what is left is the last step's three
                               roundings: (x/2) y (rel. eps/2 into the result), the fma next to 1 (eps) and the product (half an ulp):
                               0.5 + 1 + 0.5 ulp of a result just below a power of two, 1.25 ulp just above one.
  cos_sinc_tiny     0.6 ulp    c = fma(p, u, 1) with c in (0.996, 1]: its own rounding 0.5 ulp; the rounding of p (eps/4) times
                               u <= 2^-7 is 0.002 ulp, the earlier Horner steps and the rounded coefficients less; the truncation the
                               comment states, u^5/10! < 8e-18, is 0.072 ulp of eps (u^5/11! < 8e-19: 0.007 ulp for sc).  0.58 and 0.51.
  cos_sinc_small    0.75 ulp   results in [0.70, 1]: 0.5 (own rounding) + 0.62 * eps/4 = 0.155 ulp (rounding of p, times u) + 0.012
                               (the step before, times u^2) + 0.016 (1/24 as a double, times u^2) + 0.018 (the stated truncation,
                               2e-18) = 0.70 for c; 0.5 + 2 * 0.078 (q and -1/6 as a double, times u) + 0.006 + 0.018 = 0.68 for sc.
  cos_sinc_large    g^h * B    absolute; B = 0.75 eps (the small series' bound for results in [0.5, 1)), h halvings, g = 4 + 2/3.
                               c' = 2c^2 - 1 turns an error d in c into 4 c d + 2 d^2 plus one rounding (eps/2 = 2B/3), and |c| <= 1;
                               sc' = sc c turns (d_sc, d_c) into c d_sc + sc d_c plus one rounding: at most d_sc + d_c + 2B/3.  With
                               both errors <= g^(h-1) B before a halving, after it they are <= (4 g^(h-1) + 2/3) B <= g^h B for
                               g >= 4 + 2/3 (and 2 g^(h-1) + 2/3 for sc).  So the error grows by up to 4|c| per halving — 2.8 to 3.7 in
                               the first, where the reduced angle lies in (0.39, 0.79] — not by 2.
  pow_minus_fifth   4 ulp      the last Newton step y (6 - t y^5) / 5: y^5 carries 4 eps (three products), the fma next to 5 adds
                               half an ulp of 5 (4 eps): 1.6 eps relative in (6 - t y^5); then the product by y, the constant 0.2 and
                               the product by it: 4.6 eps relative if every rounding went the same way, i.e. 2.3 ulp of a result just
                               above a power of two and 4.6 just below one; the roundings do not all align (the fma's eight-eps
                               share needs t y^5 just inside a binade edge), and 4 ulp is asserted.  The step before leaves 3e-12,
                               which this step squares.
  div_1e5, u21, s21, philox4x32_10, normalized     exact: bit-equal to IEEE / integer arithmetic in NumPy.
  attitude_error_of 1 ulp      the table is the host libm's acos; the lookup itself is exact.

  For the composite functions the bound is the number R of roundings on the longest dependency chain times half an ulp of the
  result's scale (eps for unit outputs; the result itself for rms7), 16 ulp at the most:

    function                          chain                                                                     R    bound
    unit_vector                       dot3 3, rsqrt64 6 (two steps of 3), product 1                             10    5 ulp
    quat2mat                          sum of squares 4, rsqrt64 6, q inv 1, qw qw 1, inner fma 1, outer fma 1   14    7 ulp
    deviate, tiny                     inputs unit to a rounding each 2, half^2 1, series 5, sc half 1,
                                      axis s 1, product 4                                                       14    7 ulp
    deviate, not tiny (theta <= pi)   inputs 2, half^2 1, series 10, one halving 1, sc half 1, axis s 1,
                                      product 4                                                                 20   10 ulp
    integrate_attitude, tiny series   u 4 (dot3 3, product 1), series 5, sc dt/2 1, w k 1, product 4,
                                      normalisation 11 (sum of squares 4, rsqrt64 6, product 1)                 26   13 ulp
    integrate_attitude, small series  the same with the series' 10                                              31   15.5 ulp
    integrate_attitude, one halving   ... and one halving                                                       32   16 ulp
    integrate_attitude<true>, |q| rescaled   9 more (sum of squares 4, rsqrt64 6, three products instead of
                                      one ... in front of u)                                                35 - 41   16 ulp (the cap)
    rms7                              square 1, six additions 6, sqrt 1, sqrt(7.0) 1, division 1                10    5 ulp

  integrate_attitude<true> with a rescaled |q| counts more than 32 roundings: by the rule it would need more than 16 ulp.  It is held to
  16 ulp all the same; what it measures is far below (Newton steps and the final normalisation contract errors, they do not add them).
"""
import numpy as np
import pytest

import device_probe as DP
from helpers import gpu_batch, to_numpy
from reinforcement_learning_rendezvous_amd.params import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
K_TINY_U, K_SMALL_U = 0.0078125, 0.62            # rdv_device.h: kTinyU, kSmallU
B_SMALL = 0.75                                    # ulp; the bound of cos_sinc_small
B_TINY = 0.6
G_HALVING = 4.0 + 2.0 / 3.0
HALF_DT = 0.5                                     # the fixture's (make_golden_device_math.py)


@pytest.fixture(scope="module")
def probe():
    return DP.Probe()                             # (a missing librdv_probe.so raises, with the build command: no skip)


@pytest.fixture(scope="module")
def ref():
    r = DP.load_reference()
    for a in r.values():
        a.setflags(write=False)
    return r


def report(name, **figures):
    print("device_math " + name.ljust(48) + "  ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def halvings(u):
    """the trips of cos_sinc_large's loop: the smallest h with u / 4^h <= kSmallU"""
    u = np.array(u, dtype=np.float64)
    h = np.zeros(u.shape, dtype=np.int64)
    for _ in range(64):
        more = u > K_SMALL_U
        if not more.any():
            break
        u = np.where(more, u * 0.25, u)
        h += more
    return h


def unit_scale_error(got, hi, lo):
    """the absolute error in units of spacing(1.0) = 2 eps: 'ulp' of a result of scale 1"""
    return DP.abs_error(got, hi, lo) / (2.0 * EPS)


# ---------------------------------------------------------------------------------------------------------------- rsqrt64
def test_rsqrt64_within_two_ulp(probe, ref):
    x = ref["rsqrt_x"]
    assert len(x) % 2 == 1
    err = DP.ulp_error(probe.rsqrt64(x), ref["rsqrt_y_hi"], ref["rsqrt_y_lo"])
    report("rsqrt64", n=len(x), max_ulp=float(err.max()), at=float(x[err.argmax()]))
    assert err.max() <= 2.0


def test_rsqrt64_special_values(probe):
    x = np.array([0.0, np.inf, np.nan, -1.0, -np.inf, -2.5e-310, -1e300])
    y = probe.rsqrt64(x)
    assert y[0] == np.inf and y[1] == 0.0 and not np.signbit(y[1])
    assert np.isnan(y[2:]).all(), y


def test_rsqrt64_subnormal_arguments_are_reported(probe, ref):
    """x = k 2^-1074.  x/2 is exact for an even k and the 2 ulp hold; for an odd k it is rounded to an even number of units, a relative
    1/k away, and the Newton steps head for 1/sqrt(2 RN(x/2)): the result is within a relative 1/k of 1/sqrt(x) (1/(2k) from the
    argument they see, and two steps from that far do not arrive), no better.
    Can a caller pass one?  Yes: a sum of squares is subnormal when the values are below 1.5e-154, and rdv_set_state accepts a quaternion
    of such a norm (tests/test_gpu_random_params.py injects |qt| = 1.4e-160: its sum of squares is 4048 units, even).  quat2mat and
    integrate_attitude<true> then rely on a finite, positive factor that keeps the quaternion's direction — the state is renormalised
    when the step ends — not on 2 ulp; test_quat2mat_subnormal_norms measures what that costs.  A position of 1e-310 does not get
    here: its square underflows to 0 and rsqrt64(0) = inf, the reference's division by |rc| = 0."""
    x = ref["rsqrtsub_x"]
    k = x / 2.0 ** -1074
    y = probe.rsqrt64(x)
    err = DP.ulp_error(y, ref["rsqrtsub_y_hi"], ref["rsqrtsub_y_lo"])
    even = k % 2 == 0
    rel = DP.abs_error(y, ref["rsqrtsub_y_hi"], ref["rsqrtsub_y_lo"]) / ref["rsqrtsub_y_hi"]
    report("rsqrt64 subnormal, even k", n=int(even.sum()), max_ulp=float(err[even].max()))
    report("rsqrt64 subnormal, odd k", n=int((~even).sum()), max_ulp=float(err[~even].max()), max_rel_times_k=float((rel * k)[~even].max()))
    assert np.all(np.isfinite(y)) and np.all(y > 0)
    assert err[even].max() <= 2.0
    assert np.all(rel[~even] <= 1.0 / k[~even] + 4 * EPS)


# ---------------------------------------------------------------------------------------------------------------- cos_sinc
def _series(probe, ref, name, series, bound):
    u = ref[name + "_u"]
    assert len(u) % 2 == 1
    c, sc = probe.cos_sinc(u, series)
    ec = DP.ulp_error(c, ref[name + "_c_hi"], ref[name + "_c_lo"])
    es = DP.ulp_error(sc, ref[name + "_sc_hi"], ref[name + "_sc_lo"])
    report("cos_sinc_" + series, n=len(u), max_ulp_c=float(ec.max()), max_ulp_sc=float(es.max()), bound=bound)
    assert ec.max() <= bound and es.max() <= bound
    assert c[u == 0.0].tolist() == [1.0] * int((u == 0).sum()) and sc[u == 0.0].tolist() == [1.0] * int((u == 0).sum())


def test_cos_sinc_tiny_against_cos_and_sinc_of_sqrt_u(probe, ref):
    """u in [0, 2^-7], both ends: 0.6 ulp (module docstring), the truncation the header states included."""
    assert ref["tiny_u"].max() == K_TINY_U and ref["tiny_u"].min() == 0.0 and np.nextafter(K_TINY_U, 0.0) in ref["tiny_u"]
    _series(probe, ref, "tiny", "tiny", B_TINY)


def test_cos_sinc_small_against_cos_and_sinc_of_sqrt_u(probe, ref):
    """u in [0, 0.62], both ends: 0.75 ulp (module docstring)."""
    assert ref["small_u"].max() == K_SMALL_U and ref["small_u"].min() == 0.0
    _series(probe, ref, "small", "small", B_SMALL)


def test_cos_sinc_dispatcher_has_no_step_at_its_switches(probe, ref):
    """One ulp apart across kTinyU and kSmallU: the dispatcher returns the bits of the series it should take on each side, and both
    sides agree with the reference within the bound of their branch — so the step at a switch is at most the sum of the two."""
    u = ref["switch_u"]
    c, sc = probe.cos_sinc(u, "dispatch")
    tiny, small, large = (probe.cos_sinc(u, s) for s in ("tiny", "small", "large"))
    lo_side, mid, hi_side = u <= K_TINY_U, (u > K_TINY_U) & (u <= K_SMALL_U), u > K_SMALL_U
    assert lo_side.sum() >= 4 and mid.sum() >= 7 and hi_side.sum() >= 3
    for got, t, l in ((c, tiny[0], large[0]), (sc, tiny[1], large[1])):
        assert np.array_equal(got[lo_side], t[lo_side]) and np.array_equal(got[~lo_side], l[~lo_side])
    assert np.array_equal(large[0][mid], small[0][mid]) and np.array_equal(large[1][mid], small[1][mid])      # no halving up to kSmallU
    ec = DP.abs_error(c, ref["switch_c_hi"], ref["switch_c_lo"]) / EPS
    es = DP.abs_error(sc, ref["switch_sc_hi"], ref["switch_sc_lo"]) / EPS
    bound = np.where(lo_side, B_TINY, np.where(mid, B_SMALL, G_HALVING * B_SMALL))       # results in [0.5, 1): one ulp is eps
    report("cos_sinc at kTinyU", max_ulp_c=float(ec[~hi_side & (u < 0.1)].max()), max_ulp_sc=float(es[~hi_side & (u < 0.1)].max()))
    report("cos_sinc at kSmallU", max_ulp_c=float(ec[u > 0.1].max()), max_ulp_sc=float(es[u > 0.1].max()))
    assert np.all(ec <= bound) and np.all(es <= bound)


def test_cos_sinc_large_error_grows_by_at_most_g_per_halving(probe, ref):
    """u in (0.62, 1e6], 1 to 11 halvings (and some arguments below 0.62: none).  The absolute errors of c and sc per halving count h
    against g^h B, g = 4 + 2/3, B = 0.75 eps (module docstring): c = 2c^2 - 1 scales an error by 4c, so it can quadruple per halving."""
    u = ref["large_u"]
    h = halvings(u)
    assert sorted(set(h.tolist())) == list(range(12)) and u.max() == 1e6
    c, sc = probe.cos_sinc(u, "large")
    ec = DP.abs_error(c, ref["large_c_hi"], ref["large_c_lo"]) / EPS
    es = DP.abs_error(sc, ref["large_sc_hi"], ref["large_sc_lo"]) / EPS
    worst = []
    for n in range(12):
        m = h == n
        bound = G_HALVING ** n * B_SMALL
        report(f"cos_sinc_large h={n}", n=int(m.sum()), max_abs_c_in_eps=float(ec[m].max()), max_abs_sc_in_eps=float(es[m].max()), bound_in_eps=float(bound))
        worst.append((n, float(ec[m].max()), float(es[m].max()), bound))
    for n, a, b, bound in worst:
        assert a <= bound and b <= bound, (n, a, b, bound)


def test_cos_sinc_large_ends_on_infinite_and_nan_arguments(probe):
    """The halving loop is capped at 64 trips: u = inf and u = NaN come back, non-finite."""
    c, sc = probe.cos_sinc(np.array([np.inf, np.nan, np.inf]), "large")
    assert not np.isfinite(c).any() and not np.isfinite(sc).any()
    c, sc = probe.cos_sinc(np.array([np.inf, np.nan, 1.0]), "dispatch")
    assert not np.isfinite(c[:2]).any() and not np.isfinite(sc[:2]).any() and np.isfinite(c[2]) and np.isfinite(sc[2])


# ---------------------------------------------------------------------------------------------------------------- pow_minus_fifth
def test_pow_minus_fifth_within_four_ulp(probe, ref):
    x = ref["pow_x"]
    e = np.frexp(x[(x == np.ldexp(1.0, np.round(np.log2(x)).astype(np.int32)))])[1]
    assert {int(v) % 5 for v in e if v >= 0} == {0, 1, 2, 3, 4} and {int(v) % 5 for v in e if v < 0} == {0, 1, 2, 3, 4}
    assert x.min() <= 1e-8 and x.max() >= 1e13 and np.nextafter(1.0, 0.0) in x and np.nextafter(1.0, 2.0) in x
    err = DP.ulp_error(probe.pow_minus_fifth(x), ref["pow_y_hi"], ref["pow_y_lo"])
    report("pow_minus_fifth", n=len(x), max_ulp=float(err.max()), at=float(x[err.argmax()]))
    assert err.max() <= 4.0


def test_pow_minus_fifth_gives_zero_beyond_its_range(probe):
    y = probe.pow_minus_fifth(np.array([1e300, 1.5e300, 1e308, np.inf, np.nan]))
    assert y.tolist() == [0.0] * 5 and not np.signbit(y).any()


# ---------------------------------------------------------------------------------------------------------------- exact ones
def test_div_1e5_is_the_correctly_rounded_quotient(probe):
    k = np.arange(-100000, 100001, dtype=np.float64)
    got = probe.div_1e5(k)
    want = k / 1e5
    report("div_1e5", n=len(k), mismatches=int((got.view(np.uint64) != want.view(np.uint64)).sum()))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_attitude_error_of_reads_acos_to_an_ulp(probe):
    """All 200,001 entries through the device lookup: the bits of the host's table (rdv_create fills it with this expression, this libm)
    and within 1 ulp of acos(k / 1e5) at 50 digits (evaluated here: 1.6 MB of reference does not fit a committed file; ~2 s).
    |k| > 1e5 and NaN give NaN."""
    table = DP.acos_table()
    k = np.arange(-100000, 100001, dtype=np.float64)
    got = probe.attitude_error_of(table, k)
    assert np.array_equal(got.view(np.uint64), table.view(np.uint64))
    hi, lo = DP.generator().acos_reference()
    nz = hi != 0
    err = DP.ulp_error(got[nz], hi[nz], lo[nz])
    report("attitude_error_of", n=len(k), max_ulp=float(err.max()))
    assert err.max() <= 1.0 and got[~nz].tolist() == [0.0]
    bad = probe.attitude_error_of(table, np.array([100001.0, -100001.0, 1e9, -1e300, np.inf, -np.inf, np.nan]))
    assert np.isnan(bad).all()


def _spans():
    """(label, lo, span) of normalize_value's three uses: the default parameters, the nine parameter sets of
    tests/test_gpu_random_params.py, and spans whose significand is all ones or one below (nextafter(2^k, 0)), where the
    residual correction of a product by a rounded reciprocal is known to be able to miss the correctly rounded quotient."""
    from test_gpu_random_params import _random_params, _random_params_with_nominal_attitudes
    sets = [("default", make_params())]
    for case in range(9):
        rng = np.random.default_rng(1000 + case)
        sets.append((f"random{case}", _random_params(rng) if case < 6 else _random_params_with_nominal_attitudes(rng)))
    out = []
    for label, p in sets:
        for f in ("max_axial_distance", "max_axial_speed", "max_wc"):
            hi = float(getattr(p, f))
            out.append((f"{label}.{f}", -hi, hi - (-hi)))
    for k in range(-6, 9):
        a = np.nextafter(2.0 ** k, 0.0)
        for s in (a, np.nextafter(a, 0.0)):
            out.append((f"adversarial {s!r}", -s / 2, s / 2 - (-s / 2)))
    return out


def _normalized_values(rng, lo, span):
    hi = lo + span
    edge = [lo, hi, 0.0, -0.0, lo / 2, hi / 2]
    for x in (lo, hi, 0.0):
        a = b = x
        for _ in range(4):
            a, b = np.nextafter(a, -np.inf), np.nextafter(b, np.inf)
            edge += [a, b]
    huge = [s * v for s in (1.0, -1.0) for v in (1e30, 3.4028234e38, 3.5e38, 1e39, 1e100, 1e300, 4e307, 8.9e307, 9e307, 1.7e308,
                                                 np.finfo(np.float64).max, np.inf)]
    sub = [s * j * 5e-324 for s in (1.0, -1.0) for j in (1, 2, 3, 1000, 1 << 40, 1 << 51)] + [2.2250738585072014e-308, -2.2250738585072014e-308]
    parts = [np.array(edge + huge + sub),
             lo + span * rng.random(10240),                                                  # inside the Box
             (rng.random(2048) * 2 - 1) * span * np.ldexp(1.0, rng.integers(0, 40, 2048).astype(np.int32)),      # far outside
             (rng.random(1024) * 2 - 1) * np.ldexp(1.0, rng.integers(-1074, -1000, 1024).astype(np.int32)),      # subnormal and near it
             (rng.random(2048) * 2 - 1) * np.ldexp(1.0, rng.integers(100, 1024, 2048).astype(np.int32))]         # huge
    v = np.concatenate(parts)
    return np.concatenate([v, lo + span * rng.random(16385 - len(v))])


def test_normalized_is_the_references_float32_bit_for_bit(probe):
    """np.float32(2.0 * (val - lo) / span + -1.0), evaluated in float64, for 16,385 values per span: inside the Box, on its edges and
    the doubles next to them, far outside, subnormal, huge up to +-inf (a quotient that overflows is +-inf like the division's)."""
    rng = np.random.default_rng(77)
    total = wrong = 0
    for label, lo, span in _spans():
        val = _normalized_values(rng, lo, span)
        assert len(val) == 16385
        got = probe.normalized(val, lo, span, 1.0 / span)
        with np.errstate(all="ignore"):
            want = (2.0 * (val - lo) / span + -1.0).astype(np.float32)
        miss = got.view(np.uint32) != want.view(np.uint32)
        total += len(val); wrong += int(miss.sum())
        if miss.any():
            i = np.flatnonzero(miss)[:4]
            print("device_math normalized MISMATCH", label, "lo", repr(lo), "span", repr(span), "val", val[i].tolist(), "got", got[i].tolist(), "want", want[i].tolist())
    report("normalized", spans=len(_spans()), n=total, mismatches=wrong)
    assert wrong == 0


def _tie_values(rng, lo, span):
    """16,385 values whose quotient 2 (val - lo) / span, between 2^53 and 2^128 in magnitude, lies at a rounding tie of float32: val next
    to m span / 2 + lo for the midpoint m of two neighbouring floats, and the three doubles either side of it.  There an ulp of the
    numerator exceeds 1 and the float32 result turns on the last bit of the double quotient: a residual correction that is cut short
    (or a quotient that is not the correctly rounded one) shows as the neighbouring float."""
    n = 2340
    f = np.ldexp(1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23), rng.integers(53, 128, n).astype(np.int32))      # float32 values
    m = (f + np.ldexp(1.0, (np.frexp(f)[1] - 1 - 24).astype(np.int32))) * np.where(rng.random(n) < 0.5, -1.0, 1.0)   # + half a float32 ulp
    with np.errstate(over="ignore"):
        v = m * span / 2 + lo
    v = v[np.isfinite(v)]
    v = np.concatenate([v, (m * (span / 2))[: n - len(v)]])
    cols = [v]
    a = b = v
    for _ in range(3):
        a, b = np.nextafter(a, -np.inf), np.nextafter(b, np.inf)
        cols += [a, b]
    out = np.concatenate([np.stack(cols, axis=1).ravel(), [lo, lo + span, 0.0, 2.0 ** 53, -2.0 ** 53]])
    assert len(out) == 16385 and np.isfinite(out).all()
    return out


def test_normalized_at_float32_ties_of_large_quotients(probe):
    """The same equality where the correction matters most: quotients in [2^53, 2^128) placed at float32 rounding ties (_tie_values),
    for every span of _spans().  (Uniformly drawn huge values meet such a tie about once in 2^29.)"""
    rng = np.random.default_rng(78)
    total = wrong = 0
    for label, lo, span in _spans():
        val = _tie_values(rng, lo, span)
        got = probe.normalized(val, lo, span, 1.0 / span)
        with np.errstate(all="ignore"):
            quotient = 2.0 * (val - lo) / span
            want = (quotient + -1.0).astype(np.float32)
        assert (np.abs(quotient[:-5]) >= 2.0 ** 52).all()
        miss = got.view(np.uint32) != want.view(np.uint32)
        total += len(val); wrong += int(miss.sum())
        if miss.any():
            i = np.flatnonzero(miss)[:3]
            print("device_math normalized TIE MISMATCH", label, "lo", repr(lo), "span", repr(span), "val", val[i].tolist(), "got", got[i].tolist(), "want", want[i].tolist())
    report("normalized at float32 ties", spans=len(_spans()), n=total, mismatches=wrong)
    assert wrong == 0


def test_u21_and_s21_over_all_fields(probe):
    f = np.arange(1 << 21, dtype=np.uint32)
    u = (f.astype(np.float64) + 0.5) / 2097152.0
    got_u, got_s = probe.u21(f), probe.s21(f)
    report("u21 / s21", n=len(f), mismatches=int((got_u != u).sum() + (got_s != 2.0 * u - 1.0).sum()))
    assert np.array_equal(got_u.view(np.uint64), u.view(np.uint64))
    assert np.array_equal(got_s.view(np.uint64), (2.0 * u - 1.0).view(np.uint64))
    assert got_u.min() > 0 and got_u.max() < 1 and got_s.min() > -1 and got_s.max() < 1


def test_philox4x32_10_matches_the_numpy_philox(probe):
    from policy_reference import philox4x32_10
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (4096, 2), dtype=np.uint64).astype(np.uint32)
    ones = np.uint32(0xFFFFFFFF)
    ctr = np.concatenate([ctr, [[0, 0, 0, 0], [ones] * 4, [0, 0, 0, 0], [ones] * 4, [1, 0, 0, 0]]]).astype(np.uint32)
    key = np.concatenate([key, [[0, 0], [ones] * 2, [ones] * 2, [0, 0], [0, 1]]]).astype(np.uint32)
    got = probe.philox4x32_10(ctr, key)
    want = philox4x32_10([ctr[:, j] for j in range(4)], [key[:, 0], key[:, 1]])
    report("philox4x32_10", n=len(ctr), mismatches=int((got != want).sum()))
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert got[-5].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]          # Random123's known answer for zeros


# ---------------------------------------------------------------------------------------------------------------- composites
def _composite(name, got, ref, key, roundings, scale_is_result=False):
    hi, lo = ref[key + "_hi"], ref[key + "_lo"]
    err = DP.ulp_error(got, hi, lo) if scale_is_result else unit_scale_error(got, hi, lo)
    bound = min(roundings / 2.0, 16.0)
    report(name, n=len(hi), max_ulp=float(np.max(err)), bound=bound)
    assert np.max(err) <= bound
    return err


def test_unit_vector(probe, ref):
    got = probe.unit_vector(ref["unit_v"])
    _composite("unit_vector", got, ref, "unit_o", 10)
    assert np.abs((got * got).sum(axis=1) - 1.0).max() <= 8 * EPS


def test_quat2mat(probe, ref):
    """Unit, non-unit (norm 0.3 .. 13) and axis-aligned quaternions, norms of 1e-150 and 1e150."""
    q = ref["q2m_q"]
    n = np.sqrt((q * q).sum(axis=1))
    assert n.min() < 0.31 and n.max() > 12 and (np.abs(n - 1) < 1e-15).sum() > 4000
    _composite("quat2mat", probe.quat2mat(q), ref, "q2m_m", 14)


def test_quat2mat_subnormal_norms(probe, ref):
    """Quaternions of norm ~1e-160, as tests/test_gpu_random_params.py injects one: the sum of squares is k ~ 500 .. 40,000 units of
    2^-1074, rounded to a whole number of them (three roundings of up to half a unit: 1.5/k relative), and rsqrt64 of it is within
    1/k (test_rsqrt64_subnormal_arguments_are_reported): the factor is within (1.5/2 + 1)/k, the matrix — quadratic in it, entries up
    to 2 (q.q) - 1 — within 4 * 1.75/k = 7/k, plus the 7 ulp of ordinary arguments.  The reference's own q / |q| sees the same rounded
    sum: against it (the transition tests' comparison) only rsqrt64's share shows, and only for an odd k; the injected case of the
    adversarial test, [1e-160, 0, 0, 1e-160], has k = 4048, even."""
    q = ref["q2msub_q"]
    got = probe.quat2mat(q)
    err = DP.abs_error(got, ref["q2msub_m_hi"], ref["q2msub_m_lo"])
    k = (q * q).sum(axis=1) / 2.0 ** -1074
    assert k.min() > 100 and k.max() < 1e5
    report("quat2mat, |q|^2 subnormal", n=len(q), max_abs=float(err.max()), max_abs_times_k=float((err.max(axis=1) * k).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err.max(axis=1) <= 7.0 / (k - 2.0) + 14 * EPS)


def test_deviate_with_either_series(probe, ref):
    """Angles across [0, pi] with tiny = 0 (the long series, one halving beyond theta/2 = 0.787); angles up to the largest range for
    which the parameters set tiny = 1 with that setting — and the same angles with tiny = 0: at the switch both are within bounds."""
    got = probe.deviate(ref["dev_axis"], ref["dev_theta"], ref["dev_nominal"], tiny=False)
    assert ref["dev_theta"].max() == np.pi and halvings((0.5 * ref["dev_theta"]) ** 2).max() == 1
    _composite("deviate, tiny=0", got, ref, "dev_o", 20)
    t = ref["devtiny_theta"]
    assert 0.25 * t.max() * t.max() <= K_TINY_U < 0.25 * (t.max() * (1 + 1e-15)) ** 2       # derive_params' rule for tiny = 1, at its edge
    got = probe.deviate(ref["devtiny_axis"], t, ref["devtiny_nominal"], tiny=True)
    _composite("deviate, tiny=1", got, ref, "devtiny_o", 14)
    got = probe.deviate(ref["devtiny_axis"], t, ref["devtiny_nominal"], tiny=False)
    _composite("deviate, tiny=0, small angles", got, ref, "devtiny_o", 19)


def _attitude_bounds(w, extra=0):
    """roundings per element: by the series its u = (|w| dt/2)^2 selects (the larger count next to a switch)"""
    u = (w * w).sum(axis=1) * (HALF_DT * HALF_DT)
    r = np.where(u * (1 + 1e-12) <= K_TINY_U, 26, np.where(u * (1 + 1e-12) <= K_SMALL_U, 31, 32)) + extra
    assert halvings(u * (1 + 1e-12)).max() == 1
    return u, r


def test_integrate_attitude(probe, ref):
    """integrate_attitude<false> on unit quaternions: |w| dt/2 in each series' range and at both switches, w = 0 exactly."""
    q, w = ref["ia_q"], ref["ia_w"]
    got = probe.integrate_attitude(q, w, HALF_DT, raw=False)
    err = unit_scale_error(got, ref["ia_o_hi"], ref["ia_o_lo"]).max(axis=1)
    u, r = _attitude_bounds(w)
    for label, m in (("tiny", r == 26), ("small", r == 31), ("one halving", r == 32)):
        assert m.sum() > 900
        report(f"integrate_attitude<false>, {label}", n=int(m.sum()), max_ulp=float(err[m].max()), bound=float(r[m][0] / 2.0))
    assert np.all(err <= r / 2.0)
    rest = (w == 0).all(axis=1)
    assert rest.sum() == 3 and unit_scale_error(got[rest], q[rest], 0.0).max() <= 1.0       # a body at rest: q, renormalised


def test_integrate_attitude_of_an_injected_state(probe, ref):
    """integrate_attitude<true>: |q| from 1e-3 to 1e3 and |q|^2 - 1 either side of 1e-6 (beyond it the quaternion turns at w / |q|,
    within it at w), unit quaternions too.  The rates are scaled with |q| so that the angle the series sees, |w| dt/2 / |q|, lies in
    each branch with one halving at the most, as for unit quaternions: every further halving multiplies the error by up to 4 2/3
    (test_cos_sinc_large_error_grows_by_at_most_g_per_halving; an unscaled 3 rad/s on |q| = 1e-3 is 1500 rad a step, eleven halvings
    and 5860 ulp).  16 ulp throughout (the rule's count for a rescaled |q| exceeds it: module docstring)."""
    q, w = ref["iaraw_q"], ref["iaraw_w"]
    n2 = (q * q).sum(axis=1)
    assert n2.min() < 1e-5 and n2.max() > 1e5
    d = n2[3:11] - 1.0
    assert ((np.abs(d) > 1e-6) == np.array([1, 0, 1, 0, 1, 0, 1, 0], bool)).all() and np.abs(np.abs(d) - 1e-6).max() < 2e-8
    got = probe.integrate_attitude(q, w, HALF_DT, raw=True)
    err = unit_scale_error(got, ref["iaraw_o_hi"], ref["iaraw_o_lo"]).max(axis=1)
    rescaled = np.abs(n2 - 1.0) > 1e-6
    u_seen = (w * w).sum(axis=1) * (HALF_DT * HALF_DT) / np.where(rescaled, n2, 1.0)
    assert halvings(u_seen * (1 + 1e-12)).max() == 1 and (u_seen <= K_TINY_U).sum() > 600 and ((u_seen > K_TINY_U) & (u_seen <= K_SMALL_U)).sum() > 600
    report("integrate_attitude<true>, |q| rescaled", n=int(rescaled.sum()), max_ulp=float(err[rescaled].max()), bound=16.0)
    report("integrate_attitude<true>, |q| ~ 1", n=int((~rescaled).sum()), max_ulp=float(err[~rescaled].max()), bound=16.0)
    assert err.max() <= 16.0
    # on a unit quaternion the two forms are one computation
    unit = np.abs(n2 - 1.0) < 1e-15
    assert unit.sum() >= 20
    assert np.array_equal(got[unit], probe.integrate_attitude(q, w, HALF_DT, raw=False)[unit])


def test_rms7(probe, ref):
    x = ref["rms_x"]
    got = probe.rms7(x)
    hi, lo = ref["rms_y_hi"], ref["rms_y_lo"]
    assert got[hi == 0].tolist() == [0.0]
    nz = hi != 0
    err = DP.ulp_error(got[nz], hi[nz], lo[nz])
    report("rms7", n=len(x), max_ulp=float(err.max()), bound=5.0)
    assert err.max() <= 5.0


# ---------------------------------------------------------------------------------------------------------------- the product
def test_the_probe_measures_the_arithmetic_that_ships():
    """One rdv_step of 300 envs (f64 storage, halt mode, zero actions): the target quaternion it stores is, bit for bit, the probe's
    integrate_attitude<false> of the quaternion and rate before the step with dt/2 — the probe library and the product compile the
    same expression to the same arithmetic."""
    n = 300
    env = gpu_batch(n, storage="f64", on_done="halt", seed=11)
    env.reset()
    before = to_numpy(env.get_state()).copy()
    env.step(torch.zeros((n, 6), dtype=torch.float32, device="cuda"))
    after = to_numpy(env.get_state()).copy()
    half_dt = 0.5 * float(env.params.dt)
    env.close()
    want = DP.Probe().integrate_attitude(before[:, 13:17], before[:, 17:20], half_dt, raw=False)
    assert np.abs(before[:, 17:20]).max() > 0 and not np.array_equal(before[:, 13:17], after[:, 13:17])
    assert np.array_equal(after[:, 13:17].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(after[:, 17:20], before[:, 17:20])

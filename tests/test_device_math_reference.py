"""
CPU-side checks of the layer under the transition tests (no GPU): the committed 50-digit reference of the device primitives
(tests/golden/device_math_reference*.npz) is what tests/golden/make_golden_device_math.py computes, the ulp measure of
tests/device_probe.py can fail, `make` produces librdv_probe.so with exactly the expected exports, and the acos table the host fills
is within an ulp of acos.
"""
import os
import re
import subprocess

import numpy as np

import device_probe as DP
from reinforcement_learning_rendezvous_amd import _native as N

def test_committed_reference_is_what_mpmath_gives():
    """Every array regenerated (inputs from their seeds, results with mpmath at 50 digits) equals the committed one, bit for bit,
    and the files hold nothing else."""
    fresh = DP.generator().generate()
    committed = DP.load_reference()
    assert sorted(fresh) == sorted(committed)
    for name, want in fresh.items():
        got = committed[name]
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    # the encoding: lo is the rest of the value, at most half a spacing of hi, and hi + lo rounds to hi
    for name in committed:
        if name.endswith("_hi"):
            hi, lo = committed[name], committed[name[:-3] + "_lo"]
            assert np.all(np.isfinite(hi)) and np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))), name
            assert np.array_equal(hi + lo, hi), name
    for name, a in committed.items():
        assert len(a) % 2 == 1 and len(a) <= 65536, (name, len(a))       # no launch is a whole number of 256-thread blocks


def test_ulp_error_reports_a_three_ulp_perturbation_as_three_ulp():
    """The measure can fail: an expected array moved by 3 ulp is reported as 3 ulp (to within the half ulp that lo carries), an exact
    result as at most half an ulp, and the value hi + lo itself as 0."""
    ref = DP.load_reference()
    for name in ("rsqrt_y", "small_c", "pow_y", "q2m_m"):
        hi, lo = ref[name + "_hi"], ref[name + "_lo"]
        nz = hi != 0
        assert np.all(DP.ulp_error(hi, hi, lo)[nz] <= 0.5)
        assert np.array_equal(DP.ulp_error(hi, hi, np.zeros_like(lo)), np.zeros_like(hi))
        moved = hi.copy()
        for _ in range(3):
            moved = np.nextafter(moved, np.copysign(np.inf, hi))
        err = DP.ulp_error(moved, hi, lo)
        # (away from zero; a step across a power of two is two spacings of the value below it)
        same_binade = np.spacing(np.abs(moved)) == np.spacing(np.abs(hi))
        assert np.all(np.abs(err[nz & same_binade] - 3.0) <= 0.5), name
        assert np.all(err[nz] >= 2.0)
        assert np.array_equal(DP.ulp_error(moved, hi, np.zeros_like(lo))[nz & same_binade], np.full((nz & same_binade).sum(), 3.0))
        assert DP.ulp_error(moved, hi, lo).max() > 2.4                     # a bound of 2 ulp would have failed
    assert DP.abs_error(1.0 + 2.0 ** -52, 1.0, 2.0 ** -54) == 2.0 ** -52 - 2.0 ** -54


def test_make_builds_the_probe_library_with_exactly_its_exports():
    """`make` (what build() runs) links librdv_probe.so next to librdv_hip.so; it exports the probe entry points and nothing of the
    product, and the product exports nothing of the probe."""
    r = subprocess.run(["make", "-C", N.CSRC, "-j4"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(DP.LIB_PATH) and os.path.dirname(DP.LIB_PATH) == os.path.dirname(N.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", DP.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(re.findall(r" [TW] ([A-Za-z_][A-Za-z0-9_]*)\s*$", nm, re.M))
    exported = [s for s in exported if not s.startswith(("_Z", "__hip", "_init", "_fini"))]
    assert exported == DP.EXPORTS, (exported, DP.EXPORTS)
    assert not re.search(r" T rdv_", nm)
    product = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    assert "rdvprobe" not in product
    lib = DP.lib()
    for name in DP.EXPORTS:
        assert hasattr(lib, name), name
    # the Makefile compiles it with the product's flags, and `clean` removes it
    mk = open(os.path.join(N.CSRC, "Makefile")).read()
    assert "$(HIPCC) $(HIPFLAGS) -c -o $@ rdv_probe.hip" in mk
    assert re.search(r"^clean:\n\trm -f .*\$\(PROBE_OUT\)", mk, re.M)


def test_host_acos_table_is_within_an_ulp_of_acos():
    """The table attitude_error_of reads is filled by the host's libm (rdv_create; the probe's rdvprobe_fill_acos_table is the same
    expression): all 200,001 entries within 1 ulp of acos(k / 1e5) at 50 digits."""
    hi, lo = DP.generator().acos_reference()
    table = DP.acos_table()
    err = DP.ulp_error(table[hi != 0], hi[hi != 0], lo[hi != 0])
    assert err.max() <= 1.0, err.max()
    assert table[-1] == 0.0 and table[0] == np.pi and table[100000] == np.pi / 2

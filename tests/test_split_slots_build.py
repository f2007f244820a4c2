"""CPU test (no GPU): both forms of step_kernel_split<float, true> (csrc/rdv_step.h: the speculative reset and the slot form, the third
template argument) are in the gfx950 build, neither uses scratch, and both fit the 256 vector registers of two waves per SIMD, which
is what a 512-thread workgroup per CU runs at.  The report is the one tests/test_abi.py reads: `make resource`."""
import os
import re
import subprocess

from reinforcement_learning_rendezvous_amd import _native as N


def test_both_forms_of_the_split_kernel_are_built_without_scratch():
    csrc = os.path.join(os.path.dirname(N.__file__), "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()
    hipcc = var("HIPCC")
    flags = var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).replace("$(EXTRA)", "").split()
    # the first line of the Makefile's `resource` target: the translation unit that holds the one-launch step kernels
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "rdv_hip.hip"], cwd=csrc,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    report, name = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                report[name][key] = int(m.group(1))
    # Itanium mangling of <float, true, false> and <float, true, true>
    forms = {"speculative": "step_kernel_splitIfLb1ELb0EE", "slots": "step_kernel_splitIfLb1ELb1EE"}
    for form, tag in forms.items():
        hits = [k for k in report if tag in k]
        assert len(hits) == 1, f"{form}: {hits} in the resource report"
        res = report[hits[0]]
        assert res["scratch"] == 0, (form, res)
        assert res["vgprs"] + res.get("agprs", 0) <= 256, (form, res)

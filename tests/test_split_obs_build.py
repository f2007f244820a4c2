"""CPU test (no GPU): the observation form of the split step kernel, step_kernel_split_obs<float> (csrc/rdv_step.h: the target form whose
service waves also form the observation and its Box test), is in the gfx950 build exactly once, uses no scratch and fits 128 vector
registers — four waves per SIMD — and its LDS (observation rows, the two hand-overs, the two masks) lets a step and a refill workgroup
share a CU's 160 KB.  The report is the one tests/test_abi.py reads: `make resource`, the translation unit of the one-launch step kernels."""
import os
import re
import subprocess

from reinforcement_learning_rendezvous_amd import _native as N


def test_the_observation_form_is_built_once_without_scratch_within_128_registers():
    csrc = os.path.join(os.path.dirname(N.__file__), "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()
    hipcc = var("HIPCC")
    flags = var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).replace("$(EXTRA)", "").split()
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "rdv_hip.hip"], cwd=csrc,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    report, name = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                report[name][key] = int(m.group(1))
    hits = [k for k in report if "step_kernel_split_obsIfEE" in k]      # Itanium mangling of <float>
    assert len(hits) == 1, f"{hits} in the resource report"
    res = report[hits[0]]
    assert res["scratch"] == 0, res
    assert res["vgprs"] + res.get("agprs", 0) <= 128, res
    # rows 17,408 + masks 64 + R(qt) rd 6,144 + qt, wt 7,168 + the chaser half 13,312: two such workgroups fit a CU's 160 KB
    assert res["lds"] == 44096, res
    # the three forms that were there keep their names, once each (tests/test_split_target_build.py)
    for tag in ("step_kernel_splitIfLb1ELb0EE", "step_kernel_splitIfLb1ELb1EE", "step_kernel_split_targetIfEE"):
        assert len([k for k in report if tag in k]) == 1, tag

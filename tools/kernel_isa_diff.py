#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 instruction streams of two source trees (CPU-only: hipcc cross-compiles), the method of
profiles/groups_isa_diff.md: each translation unit is compiled to device assembly with the Makefile's flags; of every kernel's assembly
the comments, labels and directives are dropped, local branch labels are made anonymous, and the remaining instruction lines are
compared kernel by kernel under demangled names.  Prints a markdown table (kernel, instructions before / after, sha256 of the stream
after, identical).

    git worktree add /tmp/parent HEAD~1      # or any other checkout of the tree to compare with
    python tools/kernel_isa_diff.py /tmp/parent [--units rdv_hip rdv_policy_mlp] [--only policy_act_kernel mlp_kernel ...] > table.md

`streams(unit)` is what tests/test_policy_sets.py uses to hold the kernels of this tree to the recorded table."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = os.path.join("reinforcement_learning_rendezvous_amd", "csrc")


def hipflags(csrc):
    """HIPCC and HIPFLAGS as csrc/Makefile sets them (EXTRA empty)"""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()
    flags = var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).replace("$(EXTRA)", "")
    return var("HIPCC"), flags.split()


def assembly(csrc, unit):
    hipcc, flags = hipflags(csrc)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", out, unit + ".hip"], cwd=csrc, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1800)
        return open(out).read()


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, out)}


def kernel_streams(asm):
    """demangled kernel name -> its instruction lines (comments, labels and directives dropped, local labels anonymous)"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    streams, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                streams[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\s*\.Lfunc_end", line):
            cur = None
            continue
        code = line.split(";", 1)[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        streams[cur].append(re.sub(r"\.LBB\d+_\d+", ".L", re.sub(r"\s+", " ", code)))
    names = demangle(sorted(streams))
    return {names[k]: v for k, v in streams.items()}


def streams(unit, csrc=None):
    return kernel_streams(assembly(csrc or os.path.join(ROOT, CSRC_REL), unit))


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before", help="root of the source tree to compare with (a checkout of the parent commit)")
    ap.add_argument("--units", nargs="+", default=["rdv_hip", "rdv_policy_mlp"])
    ap.add_argument("--only", nargs="*", default=[], help="substrings of the demangled names to list (default: every kernel)")
    args = ap.parse_args()
    print("| translation unit: kernel | instructions before | instructions after | sha256 of the stream after (first 16) | identical |")
    print("|---|---|---|---|---|")
    same = total = 0
    for unit in args.units:
        a, b = streams(unit, os.path.join(args.before, CSRC_REL)), streams(unit)
        for name in sorted(set(a) | set(b)):
            if args.only and not any(w in name for w in args.only):
                continue
            la, lb = a.get(name), b.get(name)
            ok = la is not None and la == lb
            same, total = same + ok, total + 1
            print(f"| {unit}: `{name}` | {len(la) if la is not None else '-'} | {len(lb) if lb is not None else '-'} | "
                  f"`{digest(lb) if lb is not None else '-'}` | {'yes' if ok else 'NO'} |")
    print(f"\n{same} of {total} kernels identical.", file=sys.stderr)
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())

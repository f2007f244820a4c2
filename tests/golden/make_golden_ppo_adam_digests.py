#!/usr/bin/env python3
"""Writes tests/golden/ppo_adam_output_digests.json: the digests of tests/ppo_adam_digests.py computed with ANOTHER build of the library —
the one of the commit in front of a change that must keep the bits of the optimiser step.  Needs a GPU.

    git worktree add /tmp/before <commit> && make -C /tmp/before/reinforcement_learning_rendezvous_amd/csrc
    python tests/golden/make_golden_ppo_adam_digests.py /tmp/before/reinforcement_learning_rendezvous_amd/librdv_hip.so

The cases are run twice and the two runs must agree (the kernels are deterministic) before anything is written.  The fixture is never
written from the tree under test: tests/test_gpu_ppo_adam_digests.py compares this tree's build against it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
from reinforcement_learning_rendezvous_amd import _native  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    _native.LIB_PATH = os.path.abspath(sys.argv[1])
    import ppo_adam_digests
    first, second = ppo_adam_digests.digests(), ppo_adam_digests.digests()
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit(f"two runs of the same build differ in {differ}: nothing written")
    with open(os.path.join(HERE, "ppo_adam_output_digests.json"), "w") as fh:
        json.dump(first, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(first)} calls, two runs equal -> tests/golden/ppo_adam_output_digests.json")


if __name__ == "__main__":
    main()

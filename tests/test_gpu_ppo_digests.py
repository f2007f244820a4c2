"""
GPU: every output bit of rdv_ppo_loss_grad, rdv_ppo_mlp_loss_grad and rdv_ppo_set_loss_grad against tests/golden/ppo_output_digests.json,
which tests/golden/make_golden_ppo_digests.py wrote with the build of the commit in front of the one that gave the two kernel units one
definition of what they share (csrc/rdv_ppo_ops.h).  The cases and the digest are those of tests/ppo_digests.py.  A digest that differs
means a shared function changed the order of an operation: the function is mended, the fixture is not regenerated.
"""
import json
import os

import pytest

import ppo_digests

pytestmark = pytest.mark.gpu


def test_every_output_has_the_bits_of_the_build_before_the_shared_functions(golden_dir):
    with open(os.path.join(golden_dir, "ppo_output_digests.json")) as fh:
        want = json.load(fh)
    got = ppo_digests.digests()
    assert sorted(got) == sorted(want)
    assert len(got) == 8 + 2 + 4 + 4 + 5 + 4 + 1
    differ = {case: [name for name in ppo_digests.OUTPUTS if got[case][name] != want[case][name]] for case in want if got[case] != want[case]}
    assert not differ, differ

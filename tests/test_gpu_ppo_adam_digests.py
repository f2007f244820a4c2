"""
GPU: every bit that rdv_ppo_set_adam_step and rdv_ppo_mlp_set_adam_step leave in the RdvAdamState arrays and in the members' forward
blocks against tests/golden/ppo_adam_output_digests.json, which tests/golden/make_golden_ppo_adam_digests.py wrote with the build of the
commit in front of the one that gave the two calls one norm kernel and one update kernel body (csrc/rdv_ppo_adam.h).  The cases and the
digest are those of tests/ppo_adam_digests.py.  A digest that differs means the shared body changed the order of an operation: the body
is mended, the fixture is not regenerated.
"""
import json
import os

import pytest

import ppo_adam_digests as D

pytestmark = pytest.mark.gpu


def test_every_array_and_block_has_the_bits_of_the_build_before_the_shared_kernels(golden_dir):
    with open(os.path.join(golden_dir, "ppo_adam_output_digests.json")) as fh:
        want = json.load(fh)
    got = D.digests()
    assert sorted(got) == sorted(want)
    assert len(got) == 3 * 4 + 1 + 2 + 2 + 5 * 5
    differ = {call: [name for name in want[call] if got[call].get(name) != want[call][name]] for call in want if got[call] != want[call]}
    assert not differ, differ
    mlp, shipped = (got[call] for call in D.FORWARD_CASES)
    assert mlp == shipped, [name for name in shipped if mlp[name] != shipped[name]]

"""
CPU-side checks of parameter groups (include/rdv.h: one batch, several parameter sets, one launch): the host-only layout check and
its messages, the per-group parameter validation, the Python tile-table helper against a brute-force per-env map, and the resource
report of the grouped kernels.  No GPU needed.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from reinforcement_learning_rendezvous_amd import _native as N
from reinforcement_learning_rendezvous_amd.params import EnvParams, GROUP_TILE, group_tile_table, make_params


def _check(n, sizes):
    arr = (C.c_int64 * max(len(sizes), 1))(*sizes)
    rc = N.lib().rdv_param_groups_check(n, len(sizes), arr)
    return rc, N.lib().rdv_last_error().decode()


@pytest.mark.parametrize("n,sizes", [(456, [256, 200]), (968, [968]), (968, [256, 512, 200])])
def test_layouts_that_begin_every_group_on_a_tile_are_accepted(n, sizes):
    assert _check(n, sizes)[0] == 0
    assert len(group_tile_table(n, sizes)) == -(-n // GROUP_TILE)


@pytest.mark.parametrize("n,sizes,names", [
    (456, [200, 256], "group 0"),              # a group in front of the last one that ends inside a tile
    (968, [256, 512, 100], "group 2"),         # wrong sum: too few envs
    (968, [256, 512, 456], "group 2"),         # wrong sum: too many
    (968, [256, 0, 712], "group 1"),           # a zero size
    (968, [256, -256, 968], "group 1"),
    (968, [], "group 0"),                      # G = 0
])
def test_bad_layouts_are_refused_with_a_message_naming_the_group(n, sizes, names):
    rc, msg = _check(n, sizes)
    assert rc == -1 and N.ERROR_NAMES[rc] == "RDV_ERR_INVALID_ARGUMENT"
    assert names in msg, msg
    with pytest.raises(ValueError) as e:       # the Python helper raises the same errors, with the same words
        group_tile_table(n, sizes)
    assert str(e.value) == msg


def test_invalid_parameters_are_refused_naming_their_group():
    """rdv_param_groups_validate is the host-only check rdv_set_param_groups runs on its parameter sets before it touches the device."""
    lib = N.lib()
    good, bad = make_params(), make_params()
    bad.koz_radius = 1.5                         # rendezvous_env.py:155
    block = (EnvParams * 3)(good, bad, good)
    rc = lib.rdv_param_groups_validate(block, 3)
    msg = lib.rdv_last_error().decode()
    assert rc == -6 and N.ERROR_NAMES[rc] == "RDV_ERR_BAD_PARAMS"
    assert "group 1" in msg and "terminal position lies outside corridor" in msg
    assert lib.rdv_param_groups_validate((EnvParams * 3)(good, good, good), 3) == 0
    nan = make_params()
    nan.dt = float("nan")
    assert lib.rdv_param_groups_validate((EnvParams * 3)(good, good, nan), 3) == -6 and b"group 2" in lib.rdv_last_error()
    assert lib.rdv_set_param_groups(None, block, (C.c_int64 * 3)(256, 256, 256), 3, None) == -5      # bad handle, not a crash
    assert lib.rdv_num_groups(None) == -1


@pytest.mark.parametrize("n,sizes", [
    (968, [256, 512, 200]),                      # ends mid-tile, last wave has 8 envs
    (456, [256, 200]),                           # ends mid-tile
    (1024, [512, 256, 256]),
    (65536, [16384] * 4),
    (1, [1]),
])
def test_tile_table_against_a_per_env_map(n, sizes):
    per_env = np.repeat(np.arange(len(sizes)), sizes)            # brute force: the group of every env
    assert len(per_env) == n
    table = group_tile_table(n, sizes)
    assert table.dtype == np.int32 and len(table) == -(-n // GROUP_TILE)
    np.testing.assert_array_equal(table[np.arange(n) // GROUP_TILE], per_env)
    for t in range(len(table)):                                  # and no tile holds envs of two groups
        assert len(set(per_env[t * GROUP_TILE:(t + 1) * GROUP_TILE])) == 1


def test_resource_report_lists_the_grouped_kernels():
    """`make resource` covers csrc/rdv_groups.hip: every grouped kernel is in the report by name (tests/test_abi.py asserts zero scratch for
    everything in it), and the fp32 reset-by-part kernel keeps the 128 registers of step_kernel_parts<float> (four waves per SIMD)."""
    csrc = os.path.join(os.path.dirname(N.__file__), "csrc")
    r = subprocess.run(["make", "-C", csrc, "resource"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    vgprs, scratch, name = {}, {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    # the grouped step kernels are step_kernel_parts / step_kernel with the tile table's type (`const int32_t* __restrict__`: rPKi) as their
    # last template argument
    want = ["step_kernel_partsIfLb1EJrPKiE", "step_kernel_partsIfLb0EJrPKiE", "step_kernel_partsIdLb1EJrPKiE", "step_kernel_partsIdLb0EJrPKiE",
            "step_kernelIfLb1ELb0ELb0EJrPKiE", "step_kernelIfLb0ELb0ELb1EJrPKiE", "step_kernelIfLb1ELb0ELb1EJrPKiE",
            "step_kernelIdLb1ELb0ELb0EJrPKiE", "step_kernelIdLb0ELb0ELb1EJrPKiE", "step_kernelIdLb1ELb0ELb1EJrPKiE",
            "reset_kernel_groupsIf", "reset_kernel_groupsId", "access_kernel_groupsIf", "access_kernel_groupsId",
            "eval_summary_kernel_groupsIf", "eval_summary_kernel_groupsId"]
    for w in want:
        hits = [k for k in vgprs if w in k]
        assert hits, f"no kernel matching {w} in the resource report"
        assert all(scratch[k] == 0 for k in hits), (w, [scratch[k] for k in hits])
    assert max(v for k, v in vgprs.items() if "step_kernel_partsIf" in k and "EJrPKiE" in k) <= 128

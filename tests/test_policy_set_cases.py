"""
The shared comparison of tests/policy_set_cases.py, driven on the CPU (as tests/test_parity_helpers.py drives the comparator of
tests/parity.py): ``assert_columns_equal`` passes on a set's columns that ARE its members' concatenated, and raises, naming the column,
when ONE element of ONE member's column moves by one ulp (``done``: is flipped) — for every column of COLUMNS and both halves of
``lstm_state0``, in either member — and when the members come in the wrong order.  Two members of 256 and 37 rows, T = 2.
"""
import numpy as np
import pytest

from policy_set_cases import COLUMNS, assert_columns_equal

torch = pytest.importorskip("torch")

SIZES, T, H = (256, 37), 2, 8
CASES = list(COLUMNS) + ["lstm_state0 h", "lstm_state0 c"]


def _env_axis(name):
    return 0 if name in ("last_obs", "last_value") else 1


def _member(n, seed):
    """one member's collect of n envs: random float32 columns ([T, n, ...], last_obs [n, 17], last_value [n]), a random uint8 ``done``,
    ``lstm_state0`` = (h, c) [n, H]"""
    rng = np.random.default_rng(seed)
    out = {}
    for name in COLUMNS:
        shape = ((T, n) if _env_axis(name) else (n,)) + {"obs": (17,), "last_obs": (17,), "actions": (6,)}.get(name, ())
        a = rng.integers(0, 2, shape).astype(np.uint8) if name == "done" else rng.standard_normal(shape).astype(np.float32)
        out[name] = torch.from_numpy(a)
    out["lstm_state0"] = tuple(torch.from_numpy(rng.standard_normal((n, H)).astype(np.float32)) for _ in range(2))
    return out


def _pair():
    parts = [_member(n, seed=3 + g) for g, n in enumerate(SIZES)]
    got = {name: torch.cat([p[name] for p in parts], dim=_env_axis(name)) for name in COLUMNS}
    got["lstm_state0"] = tuple(torch.cat([p["lstm_state0"][i] for p in parts], dim=0) for i in range(2))
    return got, parts


def test_the_clean_pair_passes():
    got, parts = _pair()
    assert got["obs"].shape == (T, sum(SIZES), 17) and got["done"].dtype == torch.uint8 and got["last_value"].shape == (sum(SIZES),)
    assert_columns_equal(got, parts, "clean")
    assert_columns_equal(got, parts, "clean", extra=("lstm_state0",))


@pytest.mark.parametrize("member", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_one_element_of_one_member_fails_and_names_the_column(case, member):
    got, parts = _pair()
    name, _, half = case.partition(" ")
    flat = (parts[member][name]["hc".index(half)] if half else parts[member][name]).reshape(-1)      # a view of the member's own column
    i = flat.numel() - 1 if member else flat.numel() // 2
    flat[i] = 1 - flat[i] if name == "done" else torch.nextafter(flat[i], torch.tensor(np.inf, dtype=torch.float32))
    with pytest.raises(AssertionError) as e:
        assert_columns_equal(got, parts, "one ulp", extra=("lstm_state0",))
    assert f"{case}, one ulp" in str(e.value).splitlines(), str(e.value)
    if half:                                                      # the state is compared only when asked
        assert_columns_equal(got, parts, "one ulp in the state, not asked")


def test_members_in_the_wrong_order_fail():
    got, parts = _pair()
    with pytest.raises(AssertionError):
        assert_columns_equal(got, parts[::-1], "swapped", extra=("lstm_state0",))

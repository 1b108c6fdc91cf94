"""The case loop and the launcher every kernel of csrc/rt_selftest_forms.hip shares (csrc/rt_selftest_dev.h for_each_case, Tally,
launch_cases: 256 lanes a block, at most 2048 blocks, grid-stride): each self-test that takes a case table, at case counts that fill
one block partly (1, 255), two blocks and a tail (257), and one case more than the capped grid holds, so that one lane takes a
second trip (2048 * 256 + 1).  Every case runs exactly once: `tested` is the count, no mismatch appears, and -- counts being
additive -- the result is the sum of the results over a split of the same cases into two calls, which a case run twice or skipped
would break.  The cases are rows of the other tests' own edge grids and seeded generators, tiled to the count."""
import numpy as np
import pytest

import host_check
from gpu_support import abi
from test_gpu_gen_keys import cases_for
from test_gpu_pair_shadow import _walk_cases

pytestmark = pytest.mark.gpu

COUNTS = (1, 255, 257, 2048 * 256 + 1)
GEN_KEYS_SEED = 0x806AB30FD9C60ABE  # (the seed whose table has the all-zero block: "zero_blocks" is additive like the rest)


def _random_bits(seed, shape):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """name -> the rows its cases are tiled from"""
    return {
        "pair_shadow": host_check.edge_grid("pair_shadow_check", abi.PAIR_SHADOW_CASE_FLOATS, tmp_path_factory),
        "pair_shadow_walk": _walk_cases(),
        "frame_forms": host_check.edge_grid("frame_forms_check", 3, tmp_path_factory),
        "gen_keys": cases_for(GEN_KEYS_SEED),
        "short_forms": _random_bits(7, (1 << 16, 1)),   # the operands of tests/test_gpu_short_forms.py
        "div_forms": _random_bits(11, (1 << 16, 2)),    # the operand pairs of tests/test_gpu_div_forms.py
    }


# name -> (the self-test on (n, width) cases, counts of `tested` a case)
RUNNERS = {
    "pair_shadow": (lambda hb, c: hb.selftest_pair_shadow(c), 1),
    "pair_shadow_walk": (lambda hb, c: hb.selftest_pair_shadow_walk(c), 1),
    "frame_forms": (lambda hb, c: hb.selftest_frame_forms(c), 1),
    "gen_keys": (lambda hb, c: hb.selftest_gen_keys(GEN_KEYS_SEED, c), 1),
    "short_forms": (lambda hb, c: hb.selftest_short_forms(0, c[:, 0]), 4),  # each operand in four directions
    "div_forms": (lambda hb, c: hb.selftest_div_forms(operands=c), 1),
}


def _counts(res):
    """the integer counts of a result, those under "sites" by their own names; the switches' report is no count"""
    flat = {k: v for k, v in res.items() if k not in ("sites", "in_use")}
    flat.update({"site " + k: v for k, v in res.get("sites", {}).items()})
    assert flat and all(isinstance(v, int) for v in flat.values()), res
    return flat


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_every_case_runs_exactly_once(hb, rows, name, n):
    run, tested_per_case = RUNNERS[name]
    cases = np.resize(rows[name], (n, rows[name].shape[1]))  # the rows over and over, n of them
    whole = _counts(run(hb, cases))
    print(name, n, whole)
    assert whole["tested"] == tested_per_case * n, whole
    bad = {k: v for k, v in whole.items() if "mismatches" in k or k.startswith("site ")}
    assert bad and not any(bad.values()), whole
    if n > 1:
        k = n // 3
        a, b = _counts(run(hb, cases[:k])), _counts(run(hb, cases[k:]))
        assert whole == {key: a[key] + b[key] for key in whole}, (whole, a, b)

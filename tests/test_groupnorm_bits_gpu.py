"""GPU: the GroupNorm kernels' output BITS are pinned.  gn_partial_kernel / gn_finalize_kernel, gn_stats_image_kernel, gn_group_kernel,
gn_tiles_kernel and gn_apply_kernel are built from shared pieces (norm.hip; gn_group_stat in common.h also serves splitk_epilogue_gn_kernel),
so a change to one piece moves every route: each output of each case of tests/groupnorm_bits.py must reproduce the sha256 recorded in
tests/golden/groupnorm_bits.json from the library of the commit the pieces were factored out of, and -- so that the fixture cannot pin a
wrong answer -- every y must lie inside the per-element bound of tests/error_bounds.py (err/bound <= 1, the check of
tests/test_norm_bounds_gpu.py).  run_case asserts the route of every launch through ops.NORM_TRACE.  The ln_kernel cases pin the
dtype x MAXV dispatch of tt_layernorm.  A mismatch means the arithmetic changed: after an INTENDED numerical change regenerate the fixture
with tests/golden/make_groupnorm_bits.py (its docstring says how); otherwise find the change."""
import json
import os

import pytest
import torch

from tests.groupnorm_bits import CASES, case_id, run_case

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    return o


def test_the_fixture_covers_exactly_the_cases(golden):
    assert sorted(golden) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_groupnorm_output_bits(ops, golden, case):
    res = run_case(ops, case)
    for name, (sha, r) in res.items():
        print(f"{case_id(case)} {name}: sha256 {sha}, err/bound {r if r is None else format(r, '.3g')}")
    bad = {name: r for name, (_, r) in res.items() if r is not None and not r <= 1.0}
    assert not bad, f"outside the error bound (err/bound): {bad}"
    assert {name: sha for name, (sha, _) in res.items()} == golden[case_id(case)], \
        "the output bits differ from the recorded ones: the arithmetic of this route changed"

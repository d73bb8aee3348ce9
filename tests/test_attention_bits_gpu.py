"""GPU: the attention kernels' output BITS are pinned.  attn_kernel, attn_pipe_kernel and attn8_kernel are built from shared pieces
(staging, tile driver, lazy-softmax slow path, epilogue; attention.hip), so a change to one piece moves all three: every case of
tests/attention_bits.py must reproduce the sha256 recorded in tests/golden/attention_bits.json from the library of the commit the
pieces were factored out of, and -- so that the fixture cannot pin a wrong answer -- match fp32 SDPA inside the tolerance of the
neighbouring test in tests/test_ops_gpu.py.  A mismatch means the arithmetic changed: after an INTENDED numerical change regenerate
the fixture with tests/golden/make_attention_bits.py (its docstring says how); otherwise find the change."""
import json
import os

import pytest
import torch

from tests.attention_bits import CASES, case_id, output_hash, run_case

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.json")


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
def test_attention_output_bits(ops, golden, case):
    out, ref, rtol, atol = run_case(ops, case)
    got = output_hash(out)
    print(f"{case_id(case)}: sha256 {got}, max |out - SDPA| {float((out.float().cpu() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(out.float()).all())
    torch.testing.assert_close(out.float().cpu(), ref.float(), rtol=rtol, atol=atol)
    assert got == golden[case_id(case)], "the output bits differ from the recorded ones: the arithmetic of this route changed"

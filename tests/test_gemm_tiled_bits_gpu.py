"""GPU: the output BITS of the tiled GEMM template are pinned.  gemm_kernel serves every tile shape, gather mode, product form and epilogue
of tt_gemm that the persistent, streaming and big-tile kernels do not take, so a change to one of its pieces moves hundreds of instances:
every case of tests/gemm_tiled_bits.py (its docstring says what they reach, and why each shape) must reproduce the sha256 recorded in
tests/golden/gemm_tiled_bits.json from the library of the commit the pieces were factored out of, and -- so that the fixture cannot pin a
wrong answer -- match fp32 torch inside the tolerance of the family's other tests.  Each case also asserts the kernel it ran on.  The
split-K reduction kernels and sq320_kernel, which share the header, are pinned with it.  A mismatch means the arithmetic changed: after an
INTENDED numerical change regenerate the fixture with tests/golden/make_gemm_tiled_bits.py (its docstring says how); otherwise find the
change."""
import json
import os

import pytest
import torch

from tests.gemm_tiled_bits import CASES, case_id, output_hash, run_case

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_tiled_bits.json")


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
def test_gemm_tiled_output_bits(ops, golden, case):
    out, extra, ref, rtol, atol = run_case(ops, case)
    got = output_hash(out, extra)
    print(f"{case_id(case)}: sha256 {got}, max |out - fp32 torch| {float((out.float().cpu() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(out.float()).all())
    torch.testing.assert_close(out.float().cpu(), ref, rtol=rtol, atol=atol)
    assert got == golden[case_id(case)], "the output bits differ from the recorded ones: the arithmetic of this route changed"

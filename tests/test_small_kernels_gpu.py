"""GPU: every small kernel of csrc/elementwise.hip, through this_and_that_vdm_amd.ops, over the case tables of tests/small_kernels.py --
exact bits wherever the answer is exactly known, the per-element budget derived there everywhere else, canary columns beside every
strided output.  tests/test_small_kernels_cpu.py shows that these cases notice a subtly wrong kernel.  The worst err / bound per kernel
and storage type is printed when the module ends."""
import time

import pytest
import torch

from tests import small_kernels as sk

pytestmark = pytest.mark.gpu

WORST = {}
PARAMS = [pytest.param(kernel, dtype, case, id=f"{kernel}-{sk.name_of(dtype)}-{case['id']}")
          for kernel in sk.KERNELS for dtype in sk.DTYPES for case in sk.all_cases(kernel, dtype)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    t0 = time.time()
    yield o
    print(f"\n[small kernels] module time {time.time() - t0:.1f} s; worst err/bound per kernel and storage type:")
    for k, v in sorted(WORST.items()):
        print(f"[small kernels]   {k}: {v:.3g}")


@pytest.mark.parametrize("kernel,dtype,case", PARAMS)
def test_small_kernel(ops, kernel, dtype, case):
    key = f"{kernel} {sk.name_of(dtype)}"
    try:
        r = sk.run(kernel, ops, case, dtype, "cuda")
    except AssertionError:
        WORST[key] = float("inf")                        # a miss shows in the table as well
        raise
    WORST[key] = max(WORST.get(key, 0.0), r)

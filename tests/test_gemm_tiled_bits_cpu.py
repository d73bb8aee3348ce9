"""CPU: the host side of tests/gemm_tiled_bits.py.  The case ids are unique; tt_gemm_plan accepts the TtGemmArgs of every case, on the
tile and with the K split the case was written for; and the kernel name each case asserts on the GPU is tt_gemm_kernel's answer, a kernel
the library holds.  Between them the cases name every instance of gemm_kernel that is built (TT_GEMM_TILES x TT_GEMM_KMODES) and the three
of sq320_kernel.  The queries run in one child process: the library reads its knobs from the environment once."""
import json
import re
import subprocess
import sys

import pytest

from tests import gemm_route_census as census
from tests.gemm_tiled_bits import CASES, TILES, TILES_F32, case_id, kernel_of, tile_of
from tests.test_kernel_names_cpu import ROOT, symbols      # noqa: F401  (the fixture: the kernels of the loaded library)


@pytest.fixture(scope="module")
def plans():
    r = subprocess.run([sys.executable, "-m", "tests.test_gemm_tiled_bits_cpu"], cwd=ROOT, env=census.clean_env(), capture_output=True, text=True)
    assert r.returncode == 0, f"the plan queries failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.splitlines()[-1])


def test_case_ids_are_unique():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)


def test_every_case_is_planned_on_its_tile_and_names_its_kernel(plans, symbols):      # noqa: F811
    assert len(plans) == len(CASES)
    for case, (plan, (rc_name, name)) in zip(CASES, plans):
        where = f"{case_id(case)} -> {plan} {name}"
        assert plan[0] == 0 and rc_name == 0, where
        assert name == kernel_of(case) and name in symbols, where
        if case["kind"] == "sq320":
            assert plan[1:4] == [32, 320, 320], where
        else:
            assert tuple(plan[1:7]) == tile_of(case)[:6], where
        assert plan[7] == case.get("splitk", 1), where


def test_the_cases_name_every_built_instance(symbols):      # noqa: F811
    named = {kernel_of(c) for c in CASES}
    built = {s for s in symbols if re.match(r"(gemm_kernel|sq320_kernel)<", s)}
    assert len(built) == 2 * (len(TILES) * 3 + 7 * 2 + 4 + 2 * 3) + 2 * (20 + 6) + 6 and built == named, sorted(built ^ named)


if __name__ == "__main__":
    from tests.gemm_tiled_bits import plan_case
    census.load_lib()
    from this_and_that_vdm_amd import ops
    print(json.dumps([plan_case(ops, c) for c in CASES], separators=(",", ":")))

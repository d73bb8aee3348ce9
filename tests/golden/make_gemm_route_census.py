"""Writes tests/golden/gemm_route_census.json: the planner answers that tests/test_gemm_routes_cpu.py pins.

The fixture comes from a build of the library OTHER than the one under test -- the parent commit's, built in a worktree of its own:

    git worktree add ../parent <parent commit> && make -C ../parent/this_and_that_vdm_amd/csrc
    python tests/golden/make_gemm_route_census.py ../parent/this_and_that_vdm_amd/csrc/libttvdm.so

The census itself (problems, knob states, the child process without TT_* variables) is tests/gemm_route_census.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit("usage: make_gemm_route_census.py <libttvdm.so of the commit whose routes are the reference>")
    from tests.gemm_route_census import run_child
    census = run_child(os.path.abspath(sys.argv[1]))
    path = os.path.join(ROOT, "tests", "golden", "gemm_route_census.json")
    with open(path, "w") as f:
        json.dump(census, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(census['rows'])} rows, {len(census['answers'])} distinct answers, {os.path.getsize(path)} bytes")

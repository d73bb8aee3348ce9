"""Writes tests/golden/attention_refusals.json: the return codes and messages that tests/test_attention_refusals_cpu.py pins.  No GPU needed.

The fixture comes from a build of the library OTHER than the one under test -- the parent commit's, built in a worktree of its own:

    git worktree add ../parent <parent commit> && make -C ../parent/this_and_that_vdm_amd/csrc
    python tests/golden/make_attention_refusals.py ../parent/this_and_that_vdm_amd/csrc/libttvdm.so

The rows (argument families, faults, the child process that sees no GPU) are tests/attention_refusals.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit("usage: make_attention_refusals.py <libttvdm.so of the commit whose refusals are the reference>")
    from tests.attention_refusals import run_child
    codes = run_child(os.path.abspath(sys.argv[1]))
    bad = {k: v for k, v in codes.items() if v[0] not in (-1, -2)}             # TT_EINVAL / TT_EUNSUPPORTED
    assert not bad, f"rows that were not refused (a launch was attempted): {bad}"
    path = os.path.join(ROOT, "tests", "golden", "attention_refusals.json")
    with open(path, "w") as f:
        json.dump(codes, f, indent=0)
        f.write("\n")
    print(f"{path}: {len(codes)} rows")

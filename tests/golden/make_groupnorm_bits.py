"""Writes tests/golden/groupnorm_bits.json: the sha256 of every output of every case of tests/groupnorm_bits.py, which
tests/test_groupnorm_bits_gpu.py pins.  Needs the GPU.

The hashes come from a build of the library OTHER than the one under test -- the parent commit's, built in a worktree of its own and
selected with TT_LIBTTVDM (this_and_that_vdm_amd/_lib.py):

    git worktree add ../parent <parent commit> && make -C ../parent/this_and_that_vdm_amd/csrc
    TT_LIBTTVDM=../parent/this_and_that_vdm_amd/csrc/libttvdm.so python tests/golden/make_groupnorm_bits.py [output.json]

After an INTENDED numerical change of a GroupNorm / LayerNorm route (and only then) regenerate it from the changed library the same way, and
say so in the commit: a refactor must reproduce the recorded bits instead.  Every y is checked against its per-element error bound
(tests/error_bounds.py) here as well, so a wrong answer is never recorded."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    lib = os.environ.get("TT_LIBTTVDM")
    if not lib or not os.path.exists(lib):
        sys.exit("usage: TT_LIBTTVDM=<libttvdm.so of the commit whose bits are the reference> make_groupnorm_bits.py [output.json]")
    from tests.groupnorm_bits import CASES, case_id, run_case
    from this_and_that_vdm_amd import _lib, ops
    assert os.path.samefile(_lib.LIB_PATH, lib)
    golden = {}
    for case in CASES:
        res = run_case(ops, case)
        golden[case_id(case)] = {name: sha for name, (sha, _) in res.items()}
        bad = {name: r for name, (_, r) in res.items() if r is not None and not r <= 1.0}
        assert not bad, f"{case_id(case)}: outside the error bound (err/bound) {bad}"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "groupnorm_bits.json")
    with open(path, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(golden)} cases from {lib}")

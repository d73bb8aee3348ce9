"""Writes tests/golden/gemm_tiled_bits.json: the sha256 of every case of tests/gemm_tiled_bits.py, which tests/test_gemm_tiled_bits_gpu.py
pins.  Needs the GPU.

The hashes come from a build of the library OTHER than the one under test -- the parent commit's, built in a worktree of its own and
selected with TT_LIBTTVDM (this_and_that_vdm_amd/_lib.py):

    git worktree add ../parent <parent commit> && make -C ../parent/this_and_that_vdm_amd/csrc
    TT_LIBTTVDM=../parent/this_and_that_vdm_amd/csrc/libttvdm.so python tests/golden/make_gemm_tiled_bits.py [output.json]

It refuses to run without TT_LIBTTVDM or with the tree's own library.  After an INTENDED numerical change of the tiled template, its
split-K reduction or the streaming kernel (and only then) regenerate the fixture from the changed library, copied out of the tree, the
same way, and say so in the commit: a refactor must reproduce the recorded bits instead.  Every case is checked against fp32 torch here as
well, so a wrong answer is never recorded."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    lib = os.environ.get("TT_LIBTTVDM")
    own = os.path.join(ROOT, "this_and_that_vdm_amd", "csrc", "libttvdm.so")
    if not lib or not os.path.exists(lib) or (os.path.exists(own) and os.path.samefile(lib, own)):
        sys.exit("usage: TT_LIBTTVDM=<libttvdm.so of the commit whose bits are the reference, not this tree's own> make_gemm_tiled_bits.py [output.json]")
    import torch
    from tests.gemm_tiled_bits import CASES, case_id, output_hash, run_case
    from this_and_that_vdm_amd import _lib, ops
    assert os.path.samefile(_lib.LIB_PATH, lib)
    golden = {}
    for case in CASES:
        out, extra, ref, rtol, atol = run_case(ops, case)
        golden[case_id(case)] = output_hash(out, extra)
        err = (out.float().cpu() - ref).abs()
        print(f"{case_id(case)}: max |out - ref| {float(err.max()):.3e}, worst error / bound {float((err / (atol + rtol * ref.abs())).max()):.3f}", flush=True)
        torch.testing.assert_close(out.float().cpu(), ref, rtol=rtol, atol=atol)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_tiled_bits.json")
    with open(path, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(golden)} cases from {lib}")

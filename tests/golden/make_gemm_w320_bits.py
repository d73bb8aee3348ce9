"""Writes tests/golden/gemm_w320_bits.json: the sha256 of every case of tests/gemm_w320_bits.py, which tests/test_gemm_w320_bits_gpu.py pins.
Needs the GPU.

The hashes come from a build of the library OTHER than the one under test -- the parent commit's, built in a worktree of its own and
selected with TT_LIBTTVDM (this_and_that_vdm_amd/_lib.py):

    git worktree add ../parent <parent commit> && make -C ../parent/this_and_that_vdm_amd/csrc
    TT_LIBTTVDM=../parent/this_and_that_vdm_amd/csrc/libttvdm.so python tests/golden/make_gemm_w320_bits.py [output.json]

After an INTENDED numerical change of a big-tile route (and only then) regenerate it from the changed library the same way, and say so in
the commit: a refactor must reproduce the recorded bits instead.  Every case is checked against fp32 torch here as well, so a wrong answer
is never recorded."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    lib = os.environ.get("TT_LIBTTVDM")
    if not lib or not os.path.exists(lib):
        sys.exit("usage: TT_LIBTTVDM=<libttvdm.so of the commit whose bits are the reference> make_gemm_w320_bits.py [output.json]")
    import torch
    from tests.gemm_w320_bits import CASES, case_id, output_hash, run_case
    from this_and_that_vdm_amd import _lib, ops
    assert os.path.samefile(_lib.LIB_PATH, lib)
    golden = {}
    for case in CASES:
        out, sums, ref, rtol, atol = run_case(ops, case)
        golden[case_id(case)] = output_hash(out, sums)
        err = (out.float().cpu() - ref).abs()
        print(f"{case_id(case)}: max |out - ref| {float(err.max()):.3e}, worst error / bound {float((err / (atol + rtol * ref.abs())).max()):.3f}", flush=True)
        torch.testing.assert_close(out.float().cpu(), ref, rtol=rtol, atol=atol)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_w320_bits.json")
    with open(path, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(golden)} cases from {lib}")

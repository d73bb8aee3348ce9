#!/usr/bin/env python3
"""One-time cross-check: the kernel instance name ops.PROFILE records (the library's tt_gemm_kernel / tt_conv3x3_kernel /
tt_attention_kernel) is the kernel a trace sees launched.  One launch per kernel family on the small shapes of the GPU tests,
with the cases a Python copy of the dispatch used to name wrongly (sq320 with a row vector, conv3x3, split16 attention).

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/kernel_name_check.py run <dir>/recorded.json
    python tools/kernel_name_check.py compare <dir>/recorded.json <dir>          # prints the table, exit status 1 on a mismatch

Tracing only (no counters); split-K reduction passes and torch's own kernels are not profiled launches and are skipped."""
import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILIES = ("gemm_kernel", "gemm_pp_kernel", "gemm_w320_kernel", "gemm_w320h_kernel", "sq320_kernel", "conv_patch_kernel", "attn_kernel",
            "attn_pipe_kernel", "attn8_kernel")


def run(out_path):
    import torch
    from this_and_that_vdm_amd import ops
    lib = ops._lib.load()
    bf16, dev = torch.bfloat16, "cuda"
    z = lambda *shape, dtype=bf16: torch.zeros(shape, dtype=dtype, device=dev)
    labels = []

    def case(label, fn):
        n = len(ops.PROFILE)
        fn()
        assert len(ops.PROFILE) == n + 1, label
        labels.append(label)

    def attn(dtype, *, lk=128, v_rows=False, fp8=False):
        nseq, lq, heads, d = 2, 96, 2, 64
        qdt = torch.uint8 if fp8 else dtype
        q, k = z(nseq * lq, heads * d, dtype=qdt), z(nseq * lk, heads * d, dtype=qdt)
        vt = z(nseq * lk, heads * d, dtype=qdt) if v_rows else z(heads * d, nseq * lk, dtype=qdt)
        if fp8:
            q, k, vt = q.view(ops.FP8), k.view(ops.FP8), vt.view(ops.FP8)
        ops.attention(q, k, vt, z(nseq * lq, heads * d, dtype=dtype), nseq=nseq, lq=lq, heads=heads, head_dim=d, mask=0, lk=lk,
                      k_seq_stride=lk, v_seq_stride=lk, v_rows=v_rows)

    ops.PROFILE = []
    case("tiled template, Linear", lambda: ops.gemm(z(300, 128), z(192, 128)))
    case("tiled template, 3x3 conv, split-K", lambda: ops.gemm(z(252, 640), z(256, 9 * 640), mode=1, conv=(4, 7, 9, 7, 9, 1, 0)))
    case("persistent kernel", lambda: ops.gemm(z(8192 - 56, 192), z(6144, 192)))
    lib.tt_gemm_set_big_tile(2)
    case("256 x 320 big tile", lambda: ops.gemm(z(46100, 192), z(320, 192)))
    lib.tt_gemm_set_big_tile(3)
    case("128 x 320 big tile", lambda: ops.gemm(z(12500, 192), z(640, 192)))
    lib.tt_gemm_set_big_tile(1)
    lib.tt_gemm_set_streaming_square(1)
    case("sq320, residual", lambda: ops.gemm(z(4101, 320), z(320, 320), residual=z(4101, 320)))
    case("sq320, residual + row vector", lambda: ops.gemm(z(4101, 320), z(320, 320), residual=z(4101, 320),
                                                          rowvec=z(2, 320, dtype=torch.float32), rowvec_rows=1, rowvec_mod=2))
    lib.tt_gemm_set_streaming_square(2)
    case("conv3x3 (LDS patch)", lambda: ops.conv3x3(z(4 * 16 * 28, 128), z(4 * 16 * 28, 64), z(128, 9 * 192), 4, 16, 28))
    case("attention", lambda: attn(bf16))
    case("attention, v_rows, 2 key tiles", lambda: attn(bf16, v_rows=True))
    case("attention, v_rows, ragged keys", lambda: attn(bf16, lk=72, v_rows=True))
    case("attention, fp8", lambda: attn(bf16, fp8=True))
    case("attention, TT_F32 exact", lambda: attn(torch.float32))
    ops.set_f32_split(True)
    case("attention, TT_F32 split16", lambda: attn(torch.float32))
    case("tiled template, TT_F32 split16", lambda: ops.gemm(z(300, 128, dtype=torch.float32), z(192, 128, dtype=torch.float32)))
    ops.set_f32_split(False)
    torch.cuda.synchronize()
    rec, ops.PROFILE = ops.PROFILE, None
    json.dump([[label, r[0]] for label, r in zip(labels, rec)], open(out_path, "w"), indent=1)
    print(f"{len(rec)} profiled launches -> {out_path}")


def strip(sym):
    """a trace's kernel name -> no return type, parameter list, namespace qualifiers or clone suffix"""
    sym = re.sub(r"\s*\[clone [^\]]*\]$", "", sym.strip())
    depth = 0
    for i in range(len(sym) - 1, -1, -1):
        depth += sym[i] == ")"
        depth -= sym[i] == "("
        if depth == 0:
            sym = sym[:i]
            break
    return re.sub(r"(\(anonymous namespace\)|\w+)::", "", re.sub(r"^void\s+", "", sym))


def compare(rec_path, trace_dir):
    rec = json.load(open(rec_path))
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel_trace.csv under {trace_dir}, found {files}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    traced = [n for n in (strip(r["Kernel_Name"]) for r in rows) if n.split("<")[0] in FAMILIES]
    print(f"| launch | recorded by ops.PROFILE | traced | |\n|---|---|---|---|")
    bad = len(rec) != len(traced)
    for i, (label, name) in enumerate(rec):
        t = traced[i] if i < len(traced) else "(none)"
        bad |= t != name
        print(f"| {label} | `{name}` | `{t}` | {'same' if t == name else 'DIFFERENT'} |")
    print(f"{len(rec)} recorded, {len(traced)} traced launches of the profiled families: {'MISMATCH' if bad else 'all the same, in launch order'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))

#!/usr/bin/env python
"""ingest.decode_png timed against what the reference workflow does today (Pillow's ``open`` + ``load`` of every file, then one upload):
14 frames of 256 x 384 and of 576 x 1024 -- the synthetic colour field of tests/gif_reference.py with N(0, 6^2) noise (``noisy``) and
without (``smooth``) -- in files written by Pillow and by ``export.write_pngs``; one 640 x 480 noisy image; one CONSTANT 576 x 1024 frame
(Pillow's file: one chain of copies as long as the stream) beside one noisy frame of that size; and the 14 noisy 576 x 1024 files
against one of them.

  decode_png_ms   the whole call from the files' bytes (parse, two uploads, the launches, the status readback), median, wall clock
  spread_ms       the lowest and the highest of those timed calls: the run-to-run spread of the case
  inflate_us      device events around tt_png_inflate (a memset and the launches tokens, jumps x ceil(log2 stream), bytes, adler), median
  unfilter_us     device events around tt_png_unfilter, median
  kernels_us      the launches one by one: per kernel the median over --iters traced calls of its device time, the rounds of the jumps
                  summed (absent when the profiler gives none: see `kernels_note`)
  pillow_ms       Pillow's open + load of every file + one upload of the stacked frames, same process, median
  equal           the device frames equal Pillow's, byte for byte

A record, not a gate: no speed is a pass condition.  Prints one JSON line and writes it to --out (default
profiles/png_decode_bench.json)."""
import argparse
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

SIZES = [(14, 256, 384), (14, 576, 1024)]
SIGMA = 6.0
KERNELS = ("inflate_tokens_kernel", "inflate_jump_kernel", "inflate_bytes_kernel", "inflate_adler_kernel", "png_unfilter_kernel")


def events_us(fn, iters):
    for _ in range(2):
        fn()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 1)


def wall_ms(fn, iters):
    fn()                                                             # not timed: the first call of a process pays for its allocations
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3), [round(min(out), 3), round(max(out), 3)]


def inputs(n, h, w):
    from tests import gif_reference as ref
    rng = np.random.default_rng(0)
    yield "noisy", np.stack([ref.field_frame(h, w, f, SIGMA, rng) for f in range(n)], 0)
    yield "smooth", np.stack([ref.field_frame(h, w, f, 0.0, rng) for f in range(n)], 0)


def files(frames):
    from PIL import Image
    from this_and_that_vdm_amd import export
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG")
        out.append(buf.getvalue())
    yield "pillow", out
    yield "write_pngs", export.encode_png(torch.from_numpy(frames).cuda())


def pillow_decode(items):
    from PIL import Image
    out = []
    for data in items:
        im = Image.open(io.BytesIO(data))
        im.load()
        out.append(np.asarray(im))
    return np.stack(out)


def kernel_trace(fn, iters):
    """-> ({kernel: microseconds}, the median over ``iters`` traced calls of each kernel's device time; a note when the traces hold none)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        runs = []
        for _ in range(iters):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            found = {}
            for ev in prof.events():
                for k in KERNELS:
                    if k in ev.name:
                        found[k] = found.get(k, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
            if found:
                runs.append(found)
        if not runs:
            return {}, "not run: the profiler's traces held none of the kernels"
        return {k: round(statistics.median(r.get(k, 0.0) for r in runs), 1) for k in KERNELS}, None
    except Exception as e:                                           # a record, not a gate: say why the column is missing
        return {}, f"not run: {type(e).__name__}: {e}"


def row(items, iters):
    from this_and_that_vdm_amd import ingest, ops
    got = ingest.decode_png(items, "cuda")
    want = pillow_decode(items)
    out = dict(file_bytes=sum(len(d) for d in items), frames=list(got.shape), equal=bool(got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)))
    out["decode_png_ms"], out["spread_ms"] = wall_ms(lambda: ingest.decode_png(items, "cuda"), iters)
    out["pillow_ms"], out["pillow_spread_ms"] = wall_ms(lambda: torch.from_numpy(pillow_decode(items)).cuda(), iters)
    calls = []
    real_i, real_u = ops.png_inflate, ops.png_unfilter
    ops.png_inflate = lambda *a: (calls.append(a), real_i(*a))[1]
    ops.png_unfilter = lambda *a: (calls.append(a), real_u(*a))[1]
    try:
        ingest.decode_png(items, "cuda")
    finally:
        ops.png_inflate, ops.png_unfilter = real_i, real_u
    ai, au = calls[0], calls[1]
    out["inflate_us"] = events_us(lambda: real_i(*ai), iters)
    out["unfilter_us"] = events_us(lambda: real_u(*au), iters)
    trace, note = kernel_trace(lambda: (real_i(*ai), real_u(*au)), min(iters, 3))
    out["kernels_us"] = trace
    if note:
        out["kernels_note"] = note
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only the 256 x 384 size and the single files (a quick look)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_decode_bench.json"))
    a = ap.parse_args()
    rows, not_run = [], []
    for n, h, w in SIZES[:1] if a.small else SIZES:
        for name, frames in inputs(n, h, w):
            for writer, items in files(frames):
                rows.append(dict(size=[n, h, w], input=name, writer=writer, **row(items, a.iters)))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                if (h, name, writer) == (576, "noisy", "pillow"):
                    rows.append(dict(size=[1, h, w], input=name, writer=writer + ", one of the 14 files", **row(items[:1], a.iters)))
    if a.small:
        not_run.append("14 x 576 x 1024 (--small)")
    from tests import gif_reference as ref
    single = ref.field_frame(480, 640, 0, SIGMA, np.random.default_rng(1))[None]
    for writer, items in files(single):
        rows.append(dict(size=[1, 480, 640], input="noisy", writer=writer, **row(items, a.iters)))
    constant = np.full((1, 576, 1024, 3), (10, 240, 77), dtype=np.uint8)
    rows.append(dict(size=[1, 576, 1024], input="constant", writer="pillow", **row(next(files(constant))[1], a.iters)))
    noisy = next(iter(inputs(1, 576, 1024)))[1]
    rows.append(dict(size=[1, 576, 1024], input="noisy", writer="pillow", **row(next(files(noisy))[1], a.iters)))
    result = dict(tool="png_decode_bench", device=torch.cuda.get_device_name(0), iters=a.iters, rows=rows, not_run=not_run)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

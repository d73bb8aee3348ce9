#!/usr/bin/env python
"""ingest.decode_gif timed against what the reference workflow does today (imageio -> Pillow's ``open`` + ``seek`` + ``convert("RGB")``,
then an upload): 14 frames of 256 x 384 and of 576 x 1024 -- the synthetic colour field of tests/gif_reference.py with N(0, 6^2) noise
(``noisy``), without (``smooth``), and frames of one colour each (``constant``: the longest strings, every code naming the entry being
made) -- in files written by Pillow, by ``export.write_gif(lzw="host")`` and by ``write_gif(lzw="device")`` at segments of 8192 and
16384 pixels; one single-frame 640 x 480 file; and one 576 x 1024 noisy frame coded WITHOUT any clear code behind the first (a deferred
clear: one segment of the whole frame's codes, the case in which every chunk of the pixels launch rescans its segment from the start).

  decode_gif_ms   the whole call from the file's bytes (parse, two uploads, the launches, the status readback), median, wall clock
  indices_us      device events around tt_gif_decode_indices (two memsets and the launches clears, lengths, offsets, pixels), median
  compose_us      device events around tt_gif_compose, median
  kernels_us      the launches one by one: per launch the median of its device time over --iters traced calls (absent when the
                  profiler gives none: see `kernels_note`)
  pillow_ms       Pillow's open + seek + convert("RGB") of every frame + one upload of the stacked frames, same process, median
  equal           the device frames equal Pillow's, byte for byte

A record, not a gate: no speed is a pass condition.  Prints one JSON line and writes it to --out (default
profiles/gif_decode_bench.json)."""
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
KERNELS = ("gif_clears_kernel", "gif_lengths_kernel", "gif_offsets_kernel", "gif_pixels_kernel", "gif_compose_kernel")


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
    return round(statistics.median(out), 3)


def inputs(n, h, w):
    from tests import gif_reference as ref
    rng = np.random.default_rng(0)
    yield "noisy", np.stack([ref.field_frame(h, w, f, SIGMA, rng) for f in range(n)], 0)
    yield "smooth", np.stack([ref.field_frame(h, w, f, 0.0, rng) for f in range(n)], 0)
    yield "constant", np.stack([np.full((h, w, 3), (10 + 17 * f, 240 - 13 * f, 7 * f), dtype=np.uint8) for f in range(n)], 0)


def files(frames):
    from PIL import Image
    from this_and_that_vdm_amd import export
    imgs = [Image.fromarray(f) for f in frames]
    buf = io.BytesIO()
    imgs[0].save(buf, format="GIF", save_all=len(imgs) > 1, append_images=imgs[1:], duration=50, loop=0)
    yield "pillow", buf.getvalue()
    dev = torch.from_numpy(frames).cuda()
    for name, kw in (("write_gif host", dict(lzw="host")), ("write_gif device 8192", dict(lzw="device", segment=8192)),
                     ("write_gif device 16384", dict(lzw="device", segment=16384))):
        buf = io.BytesIO()
        export.write_gif(dev, buf, duration=0.05, **kw)
        yield name, buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


def kernel_trace(fn, iters):
    """-> ({kernel: microseconds}, the median over ``iters`` traced calls of each launch's device time; a note when the traces hold none)"""
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


def row(data, iters):
    from this_and_that_vdm_amd import ingest, ops
    got = ingest.decode_gif(data, "cuda")
    want = pillow_decode(data)
    out = dict(file_bytes=len(data), frames=list(got.shape), equal=bool(got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)))
    out["decode_gif_ms"] = wall_ms(lambda: ingest.decode_gif(data, "cuda"), iters)
    out["pillow_ms"] = wall_ms(lambda: torch.from_numpy(pillow_decode(data)).cuda(), iters)
    calls = []
    real_i, real_c = ops.gif_indices, ops.gif_compose
    ops.gif_indices = lambda *a: (calls.append(("i", a)), real_i(*a))[1]
    ops.gif_compose = lambda *a: (calls.append(("c", a)), real_c(*a))[1]
    try:
        ingest.decode_gif(data, "cuda")
    finally:
        ops.gif_indices, ops.gif_compose = real_i, real_c
    ai, ac = calls[0][1], calls[1][1]
    out["indices_us"] = events_us(lambda: real_i(*ai), iters)
    out["compose_us"] = events_us(lambda: real_c(*ac), iters)
    trace, note = kernel_trace(lambda: (real_i(*ai), real_c(*ac)), iters)
    out["kernels_us"] = trace
    if note:
        out["kernels_note"] = note
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only the 256 x 384 size and the single file (a quick look)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gif_decode_bench.json"))
    a = ap.parse_args()
    rows, not_run = [], []
    for n, h, w in SIZES[:1] if a.small else SIZES:
        for name, frames in inputs(n, h, w):
            for writer, data in files(frames):
                rows.append(dict(size=[n, h, w], input=name, writer=writer, **row(data, a.iters)))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if a.small:
        not_run.append("14 x 576 x 1024 (--small)")
    from tests import gif_reference as ref
    single = ref.field_frame(480, 640, 0, SIGMA, np.random.default_rng(1))[None]
    for writer, data in list(files(single))[:2]:
        rows.append(dict(size=[1, 480, 640], input="noisy", writer=writer, **row(data, a.iters)))
    # one frame, one segment: the writer of tests/gif_decode_reference.py with a deferred clear, on the first noisy frame's own indices
    from tests import gif_decode_reference as g
    from this_and_that_vdm_amd import export
    big = next(iter(inputs(1, 576, 1024)))[1]
    q = export.quantize_frames(torch.from_numpy(big).cuda())
    for deferred in (False, True):
        data = g.gif_file(1024, 576, [dict(indices=q.indices[0], deferred=deferred, min_code_size=8)], global_table=q.palettes[0][:int(q.ncolors[0])])
        rows.append(dict(size=[1, 576, 1024], input="noisy", writer="handwritten, deferred clear" if deferred else "handwritten, a clear at every full table",
                         **row(data, a.iters)))
    result = dict(tool="gif_decode_bench", device=torch.cuda.get_device_name(0), iters=a.iters, rows=rows, not_run=not_run)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

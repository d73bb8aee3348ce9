#!/usr/bin/env python
"""export.write_gif timed against what the reference workflow does today (imageio -> Pillow's ``save(save_all=True)``): 14 frames of
256 x 384 and of 576 x 1024, the synthetic colour field of tests/gif_reference.py (frame numbers 0 .. 13) plus N(0, 6^2) noise.

  pillow_ms          Pillow's Image.save(format="GIF", save_all=True) from host uint8 frames, on this machine's CPU (wall clock, one run)
  write_gif_host_ms  export.write_gif from the same host frames (upload included), median of --iters, wall clock around a synchronised call
  write_gif_dev_ms   export.write_gif from frames that are on the device already
  stages             the new path taken apart (device frames; `upload_ms` is what host frames add):
                       hist_kernel_us / map_kernel_us / map_stats_kernel_us   device events around the launch (memsets included)
                       hist_readback_ms, median_cut_ms, palette_upload_ms, result_readback_ms, lzw_ms, container_ms   host clock
  bytes              the files' sizes
  psnr               each path's per-video PSNR to the source (Pillow's from its decoded file)
  refine4            write_gif with refine=4: time, size, PSNR

With ``--lzw device`` the tool measures the LZW stage's device route instead (tt_gif_lzw_frames; export.write_gif(lzw="device")), next
to the host coder timed in the same process, on the noisy frames above and on the smooth field without noise, once per ``--segment``
(default 4096, 8192, 16384, 32768):

  host               lzw_ms (tt_gif_lzw over the frames, host clock), write_gif_ms and the file's bytes on the host route
  per segment        lzw_device_ms (device events around the launches of ops.gif_lzw, median), readback_ms (lengths, then the bytes in
                     use), write_gif_ms (the whole call, lzw="device"), bytes_to_host (what those two readbacks move), bytes (the
                     file) and its growth over the host route's file

A record, not a gate.  Prints one JSON line and writes it to --out (default profiles/gif_export_bench.json, or
profiles/gif_lzw_device_bench.json with ``--lzw device``)."""
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


def events_us(fn, iters):
    for _ in range(3):
        fn()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def wall_ms(fn, iters):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def video_psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def pillow_save(frames):
    from PIL import Image, ImageSequence
    imgs = [Image.fromarray(f) for f in frames]
    buf = io.BytesIO()
    t0 = time.perf_counter()
    imgs[0].save(buf, format="GIF", save_all=True, append_images=imgs[1:], duration=50, loop=0)
    ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for im in imgs:
        im.quantize(256)                                  # what save() spends on the palettes (its default method for RGB)
    q_ms = (time.perf_counter() - t0) * 1e3
    back = np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(io.BytesIO(buf.getvalue())))], 0)
    return ms, q_ms, len(buf.getvalue()), video_psnr(back, frames)


def stages(dev, host, iters):
    from this_and_that_vdm_amd import export, ops
    out = dict(upload_ms=wall_ms(lambda: torch.from_numpy(host).cuda(), iters))
    out["hist_kernel_us"] = events_us(lambda: ops.color_hist(dev), iters)
    hist_dev = ops.color_hist(dev)
    out["hist_readback_ms"] = wall_ms(lambda: hist_dev.cpu(), iters)
    hist = hist_dev.cpu().numpy()
    t0 = time.perf_counter()
    cut = [export.median_cut(h) for h in hist]
    out["median_cut_ms"] = (time.perf_counter() - t0) * 1e3
    palettes = np.stack([p for p, _ in cut], 0)
    ncolors = [k for _, k in cut]
    out["palette_upload_ms"] = wall_ms(lambda: torch.from_numpy(palettes).cuda(), iters)
    pal_dev = torch.from_numpy(palettes).cuda()
    out["map_kernel_us"] = events_us(lambda: ops.palette_map(dev, pal_dev, ncolors), iters)
    out["map_stats_kernel_us"] = events_us(lambda: ops.palette_map(dev, pal_dev, ncolors, stats=True), iters)
    idx, sse, _ = ops.palette_map(dev, pal_dev, ncolors)
    out["result_readback_ms"] = wall_ms(lambda: torch.cat([idx.reshape(-1), sse.view(torch.uint8)]).cpu(), iters)
    idx_h = idx.cpu().numpy()
    t0 = time.perf_counter()
    for f in idx_h:
        export.lzw_frame(f, 8)
    out["lzw_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    export.write_gif_indexed(idx_h, palettes, ncolors, io.BytesIO())
    out["container_ms"] = (time.perf_counter() - t0) * 1e3 - out["lzw_ms"]
    return {k: round(v, 3) for k, v in out.items()}


def lzw_device_rows(iters, segments):
    """the device route of the LZW stage per input and segment size, next to the host coder in the same process"""
    from tests import gif_reference as ref
    from this_and_that_vdm_amd import export, ops
    rows = []
    for n, h, w in SIZES:
        for name, sigma in (("noisy", SIGMA), ("smooth", 0.0)):
            rng = np.random.default_rng(0)
            dev = torch.from_numpy(np.stack([ref.field_frame(h, w, f, sigma, rng) for f in range(n)], 0)).cuda()
            buf = io.BytesIO()
            q = export.write_gif(dev, buf, duration=0.05)
            sizes = [max(2, int(c - 1).bit_length()) for c in q.ncolors]
            idx = torch.from_numpy(q.indices).cuda()

            def host_lzw():
                for f, m in zip(q.indices, sizes):
                    export.lzw_frame(f, m)

            row = dict(frames=[n, h, w, 3], input=name,
                       host=dict(lzw_ms=round(wall_ms(host_lzw, iters), 3), write_gif_ms=round(wall_ms(lambda: export.write_gif(dev, io.BytesIO()), iters), 2),
                                 bytes=len(buf.getvalue())), segments=[])
            for seg in segments:
                out = io.BytesIO()
                export.write_gif(dev, out, duration=0.05, lzw="device", segment=seg)
                data, lengths, _ = ops.gif_lzw(idx, sizes, seg)
                used = int(lengths.max())

                def readback():
                    top = int(lengths.cpu().max())
                    data[:, :top].cpu()

                row["segments"].append(dict(
                    segment=seg, lzw_device_ms=round(events_us(lambda: ops.gif_lzw(idx, sizes, seg), iters) / 1e3, 3), readback_ms=round(wall_ms(readback, iters), 3),
                    write_gif_ms=round(wall_ms(lambda: export.write_gif(dev, io.BytesIO(), lzw="device", segment=seg), iters), 2),
                    bytes_to_host=8 * n + n * used, bytes=len(out.getvalue()),
                    growth_percent=round(100.0 * (len(out.getvalue()) - len(buf.getvalue())) / len(buf.getvalue()), 2)))
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true", help="skip Pillow's side")
    ap.add_argument("--lzw", choices=("host", "device"), default="host", help="device: measure the LZW stage's device route (see above)")
    ap.add_argument("--segment", type=int, action="append", help="with --lzw device: a segment size to measure (repeatable)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "gif_lzw_device_bench.json" if a.lzw == "device" else "gif_export_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("gif_export_bench: needs a GPU (there is no CPU fallback)")
    if a.lzw == "device":
        res = dict(tool="gif_export_bench --lzw device", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), iters=a.iters,
                   inputs=f"the colour field of tests/gif_reference.py, frames 0 .. 13: noisy = plus N(0, {SIGMA:g}^2) noise, smooth = without",
                   rows=lzw_device_rows(a.iters, a.segment or [4096, 8192, 16384, 32768]),
                   says="a record, not a gate; lzw_device_ms is device events around ops.gif_lzw (allocations and the launches), the rest the host "
                        "clock around synchronised calls; the host coder is timed in the same process")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    from tests import gif_reference as ref
    from this_and_that_vdm_amd import export
    rows = []
    for n, h, w in SIZES:
        rng = np.random.default_rng(0)
        host = np.stack([ref.field_frame(h, w, f, SIGMA, rng) for f in range(n)], 0)
        dev = torch.from_numpy(host).cuda()
        export.write_gif(dev, io.BytesIO())                # warm-up: library load, workspace, first launches
        row = dict(frames=[n, h, w, 3])
        for name, src in (("host", host), ("dev", dev)):
            row[f"write_gif_{name}_ms"] = round(wall_ms(lambda: export.write_gif(src, io.BytesIO(), duration=0.05), a.iters), 2)
        buf = io.BytesIO()
        q = export.write_gif(dev, buf, duration=0.05)
        row.update(bytes=len(buf.getvalue()), psnr=round(q.psnr, 3), stages=stages(dev, host, a.iters))
        buf = io.BytesIO()
        qg = export.write_gif(dev, buf, duration=0.05, palette="global")
        row["global_palette"] = dict(write_gif_dev_ms=round(wall_ms(lambda: export.write_gif(dev, io.BytesIO(), palette="global"), a.iters), 2),
                                     bytes=len(buf.getvalue()), psnr=round(qg.psnr, 3))
        buf = io.BytesIO()
        q4 = export.write_gif(dev, buf, duration=0.05, refine=4)
        row["refine4"] = dict(write_gif_dev_ms=round(wall_ms(lambda: export.write_gif(dev, io.BytesIO(), refine=4), a.iters), 2),
                              write_gif_host_ms=round(wall_ms(lambda: export.write_gif(host, io.BytesIO(), refine=4), a.iters), 2),
                              bytes=len(buf.getvalue()), psnr=round(q4.psnr, 3))
        if not a.no_pillow:
            ms, q_ms, size, p = pillow_save(host)
            row["pillow"] = dict(save_ms=round(ms, 1), quantize_ms=round(q_ms, 1), bytes=size, psnr=round(p, 3))
            row["faster_than_pillow"] = dict(host=bool(row["write_gif_host_ms"] < ms), dev=bool(row["write_gif_dev_ms"] < ms),
                                             refine4_host=bool(row["refine4"]["write_gif_host_ms"] < ms))
        rows.append(row)
    import PIL
    res = dict(tool="gif_export_bench", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), pillow=PIL.__version__,
               iters=a.iters, inputs=f"the colour field of tests/gif_reference.py, frames 0 .. 13, plus N(0, {SIGMA:g}^2) noise", rows=rows,
               says="a record, not a gate; Pillow runs once, on this machine's CPU; kernel times are device events, the rest the host clock")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

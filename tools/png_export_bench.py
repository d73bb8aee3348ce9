#!/usr/bin/env python
"""export.write_pngs timed against what the reference workflow does today (``frame.save(str(idx) + ".png")`` per frame, Pillow on one
thread): 14 frames of 256 x 384 and of 576 x 1024 from the generator of tests/png_reference.py (smooth sinusoids, N(0, 3^2) noise, one
flat rectangle; seeds 0 .. 13).

  pillow_ms            Pillow's Image.save(path) for the 14 host frames into a temporary folder, on this machine's CPU (wall clock, one run)
  write_pngs_host_ms   export.write_pngs from the same host frames (upload included), median of --iters, wall clock around the call
  write_pngs_dev_ms    export.write_pngs from frames that are on the device already
  stages               the new path taken apart (device frames; `upload_ms` is what host frames add):
                         filter_kernel_us / tokens_kernel_us / emit_kernel_us          device events around the launch
                         records_readback_ms, plan_ms (code lengths, headers, tables: host), tables_upload_ms, streams_readback_ms,
                         adler_and_slices_ms (the per-frame stream assembled on the host), crc_and_chunks_ms (the files in memory),
                         file_write_ms                                               host clock
  bytes                the 14 files' sizes, this library's and Pillow's, and their ratio; stream_over_pixels: compressed stream / pixels

A record, not a gate.  Prints one JSON line and writes it to --out (default profiles/png_export_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

SIZES = [(14, 256, 384), (14, 576, 1024)]


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


def pillow_save(frames, folder):
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames]
    t0 = time.perf_counter()
    for i, im in enumerate(imgs):
        im.save(os.path.join(folder, f"{i}.png"))
    ms = (time.perf_counter() - t0) * 1e3
    return ms, sum(os.path.getsize(os.path.join(folder, f"{i}.png")) for i in range(len(imgs)))


def stages(dev, host, folder, iters):
    from this_and_that_vdm_amd import export, ops
    shape = tuple(dev.shape[1:])
    out = dict(upload_ms=wall_ms(lambda: torch.from_numpy(host).cuda(), iters))
    out["filter_kernel_us"] = events_us(lambda: ops.png_filter(dev, 5), iters)
    filtered = ops.png_filter(dev, 5)
    out["tokens_kernel_us"] = events_us(lambda: ops.png_tokens(filtered, shape), iters)
    records = ops.png_tokens(filtered, shape)
    out["records_readback_ms"] = wall_ms(lambda: records.cpu(), iters)
    rec = records.cpu().numpy()
    out["plan_ms"] = wall_ms(lambda: export.png_plan(rec), iters)
    tables, headers, total = export.png_plan(rec)
    out["tables_upload_ms"] = wall_ms(lambda: (torch.from_numpy(tables).cuda(), torch.from_numpy(headers).cuda()), iters)
    tab_dev, hdr_dev = torch.from_numpy(tables).cuda(), torch.from_numpy(headers).cuda()
    out["emit_kernel_us"] = events_us(lambda: ops.png_emit(filtered, shape, tab_dev, hdr_dev, total), iters)
    stripes = ops.png_emit(filtered, shape, tab_dev, hdr_dev, total)
    out["streams_readback_ms"] = wall_ms(lambda: stripes.cpu(), iters)
    whole = wall_ms(lambda: export.png_streams(dev), iters)
    known = out["filter_kernel_us"] / 1e3 + out["tokens_kernel_us"] / 1e3 + out["emit_kernel_us"] / 1e3 + out["records_readback_ms"] + out["plan_ms"] \
        + out["tables_upload_ms"] + out["streams_readback_ms"]
    out["adler_and_slices_ms"] = max(0.0, whole - known)
    s = export.png_streams(dev)
    out["crc_and_chunks_ms"] = wall_ms(lambda: export.png_files(s), iters)
    files = export.png_files(s)

    def write():
        for i, data in enumerate(files):
            with open(os.path.join(folder, f"{i}.png"), "wb") as fh:
                fh.write(data)
    out["file_write_ms"] = wall_ms(write, iters)
    out["stream_bytes"] = int(total)
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true", help="skip Pillow's side")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_export_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_export_bench: needs a GPU (there is no CPU fallback)")
    from PIL import Image
    from tests import png_reference as ref
    from this_and_that_vdm_amd import export
    rows = []
    for n, h, w in SIZES:
        host = np.stack([ref.generator_frame(h, w, f) for f in range(n)], 0)
        dev = torch.from_numpy(host).cuda()
        with tempfile.TemporaryDirectory() as folder:
            paths = export.write_pngs(dev, folder)            # warm-up: library load, first launches -- and the files checked once
            for p, want in zip(paths, host):
                with Image.open(p) as im:
                    assert np.array_equal(np.asarray(im), want), p
            row = dict(frames=[n, h, w, 3])
            for name, src in (("host", host), ("dev", dev)):
                row[f"write_pngs_{name}_ms"] = round(wall_ms(lambda: export.write_pngs(src, folder), a.iters), 2)
            size = sum(os.path.getsize(p) for p in paths)
            row.update(bytes=size, stages=stages(dev, host, folder, a.iters))
            row["stream_over_pixels"] = round(row["stages"]["stream_bytes"] / host.size, 4)
            if not a.no_pillow:
                ms, psize = pillow_save(host, folder)
                row["pillow"] = dict(save_ms=round(ms, 1), bytes=psize)
                row["bytes_over_pillow"] = round(size / psize, 4)
                row["faster_than_pillow"] = dict(host=bool(row["write_pngs_host_ms"] < ms), dev=bool(row["write_pngs_dev_ms"] < ms))
        rows.append(row)
    import PIL
    res = dict(tool="png_export_bench", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), pillow=PIL.__version__,
               iters=a.iters, inputs="the generator of tests/png_reference.py, seeds 0 .. 13", rows=rows,
               says="a record, not a gate; Pillow runs once, on this machine's CPU; kernel times are device events, the rest the host clock; "
                    "files go to a temporary folder")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

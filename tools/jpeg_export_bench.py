#!/usr/bin/env python
"""export.write_jpegs timed against Pillow's per-frame ``save(format="JPEG", quality=75)`` (libjpeg-turbo, SIMD, one thread) and against the
project's own export.write_pngs on the same frames: 14 frames of 256 x 384 and of 576 x 1024 from the generator of tests/png_reference.py
(smooth sinusoids, N(0, 3^2) noise, one flat rectangle; seeds 0 .. 13).  Quality 75, 4:2:0, the standard Huffman tables -- Pillow's
defaults --, so both sides write the same bytes (checked once per size).

  pillow_ms             Pillow's Image.save(path, quality=75) for the 14 host frames into a temporary folder (median of --iters, wall clock)
  write_jpegs_host_ms   export.write_jpegs from the same host frames (upload included), median of --iters, wall clock around the call
  write_jpegs_dev_ms    export.write_jpegs from frames that are on the device already
  write_jpegs_dev_optimized_ms   ... with huffman="optimized" (one more readback, the tables made on the host)
  write_pngs_dev_ms     export.write_pngs from the same device frames
  stages                coeffs_kernel_us / counts_and_coeffs_kernel_us / scan_kernels_us: device events around the launches;
                        readback_ms (lengths, then the packed scans), files_ms (headers joined to the scans), file_write_ms: host clock
  bytes                 the 14 files' sizes (JPEG, optimized JPEG, Pillow's JPEG, this library's PNG) and what crosses to the host

  --restart-rows N      instead: export.write_jpegs from the device frames without markers and with ``restart_rows=N`` in ONE process, the
                        scan kernels of both by device events, and the files' sizes: the overhead is exact (DRI 6 bytes a file; per marker 2
                        bytes, the pad to a byte, a stuffed pad now and then, and the DC differences that start again from 0).  The result
                        goes under "encode" of profiles/jpeg_restart_bench.json (tools/jpeg_decode_bench.py fills "decode").

A record, not a gate.  Prints one JSON line and writes it to --out (default profiles/jpeg_export_bench.json)."""
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


def pillow_save(frames, folder, iters):
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames]

    def save():
        for i, im in enumerate(imgs):
            im.save(os.path.join(folder, f"pil_{i}.jpg"), quality=75)
    save()
    return wall_ms(save, iters), [os.path.join(folder, f"pil_{i}.jpg") for i in range(len(imgs))]


def stages(dev, folder, iters):
    from this_and_that_vdm_amd import export, ops
    shape = tuple(dev.shape[1:])
    out = dict(coeffs_kernel_us=events_us(lambda: ops.jpeg_coeffs(dev, 75, "4:2:0", counts=False), iters),
               counts_and_coeffs_kernel_us=events_us(lambda: ops.jpeg_coeffs(dev, 75, "4:2:0", counts=True), iters))
    coeffs, _ = ops.jpeg_coeffs(dev, 75, "4:2:0", counts=False)
    standard = export.jpeg_standard_tables()
    tables = torch.from_numpy(np.stack([t.codes for t in standard]).view(np.int32)[None]).cuda()
    out["scan_kernels_us"] = events_us(lambda: ops.jpeg_scan(coeffs, shape, "4:2:0", tables), iters)
    scans, lengths = ops.jpeg_scan(coeffs, shape, "4:2:0", tables)

    def readback():
        lens = lengths.cpu().numpy()
        return lens, torch.cat([scans[i, :int(lens[i])] for i in range(len(lens))]).cpu().numpy()
    out["readback_ms"] = wall_ms(readback, iters)
    lens, packed = readback()
    ends = np.cumsum(lens)
    n, h, w, ch = dev.shape

    def files():
        return [export.jpeg_file(packed[int(e - k):int(e)].tobytes(), h, w, ch, 75, "4:2:0", standard) for e, k in zip(ends, lens)]
    out["files_ms"] = wall_ms(files, iters)
    data = files()

    def write():
        for i, d in enumerate(data):
            with open(os.path.join(folder, f"stage_{i}.jpg"), "wb") as fh:
                fh.write(d)
    out["file_write_ms"] = wall_ms(write, iters)
    return {k: round(v, 3) for k, v in out.items()}, int(lens.sum()) + 4 * n


def restart_main(a):
    from tests import png_reference as ref
    from this_and_that_vdm_amd import export, ops
    from tools.jpeg_decode_bench import merge_out
    rows = []
    tables = torch.from_numpy(np.stack([t.codes for t in export.jpeg_standard_tables()]).view(np.int32)[None]).cuda()
    for n, h, w in SIZES:
        dev = torch.from_numpy(np.stack([ref.generator_frame(h, w, f) for f in range(n)], 0)).cuda()
        ri = a.restart_rows * ((w + 15) // 16)
        coeffs, _ = ops.jpeg_coeffs(dev, 75, "4:2:0", counts=False)
        with tempfile.TemporaryDirectory() as folder:
            export.write_jpegs(dev, folder)                    # warm-up: library load, first launches
            export.write_jpegs(dev, folder, restart_rows=a.restart_rows)
            row = dict(frames=[n, h, w, 3], restart_interval=ri, markers_per_frame=((h + 15) // 16 * ((w + 15) // 16) + ri - 1) // ri - 1)
            for name, kw in (("plain", {}), ("marked", dict(restart_rows=a.restart_rows))):
                sizes = [len(d) for d in export.encode_jpeg(dev, **kw)]
                row[name] = dict(write_jpegs_dev_ms=round(wall_ms(lambda: export.write_jpegs(dev, folder, **kw), a.iters), 2),
                                 scan_kernels_us=round(events_us(lambda: ops.jpeg_scan(coeffs, (h, w, 3), "4:2:0", tables, restart_interval=ri if kw else 0), a.iters), 1),
                                 file_bytes=int(sum(sizes)))
            row["extra_bytes"] = row["marked"]["file_bytes"] - row["plain"]["file_bytes"]
            row["extra_bytes_per_marker"] = round((row["extra_bytes"] - 6 * n) / max(1, n * row["markers_per_frame"]), 2)
            row["slower"] = bool(row["marked"]["write_jpegs_dev_ms"] > row["plain"]["write_jpegs_dev_ms"])
        rows.append(row)
    res = dict(tool="jpeg_export_bench --restart-rows", restart_rows=a.restart_rows, device=torch.cuda.get_device_name(0), iters=a.iters,
               inputs="the generator of tests/png_reference.py, seeds 0 .. 13; quality 75, 4:2:0, standard tables", rows=rows,
               says="a record, not a gate; medians of --iters in one process after a warm-up; kernel times are device events, the rest the host clock; "
                    "files go to a temporary folder; the sizes are exact")
    merge_out(a.out, "encode", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--restart-rows", type=int, default=0, metavar="N", help="compare write_jpegs(restart_rows=N) against the marker-less call")
    ap.add_argument("--out", default=None, help="default profiles/jpeg_export_bench.json; with --restart-rows profiles/jpeg_restart_bench.json")
    a = ap.parse_args()
    a.out = a.out or os.path.join(REPO, "profiles", "jpeg_restart_bench.json" if a.restart_rows else "jpeg_export_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_export_bench: needs a GPU (there is no CPU fallback)")
    if a.restart_rows:
        return restart_main(a)
    from tests import png_reference as ref
    from this_and_that_vdm_amd import _lib, export
    rows = []
    for n, h, w in SIZES:
        host = np.stack([ref.generator_frame(h, w, f) for f in range(n)], 0)
        dev = torch.from_numpy(host).cuda()
        with tempfile.TemporaryDirectory() as folder:
            paths = export.write_jpegs(dev, folder)           # warm-up: library load, first launches
            export.write_pngs(dev, os.path.join(folder, "png"))
            row = dict(frames=[n, h, w, 3], raw_bytes=int(host.size))
            for name, src in (("host", host), ("dev", dev)):
                row[f"write_jpegs_{name}_ms"] = round(wall_ms(lambda: export.write_jpegs(src, folder), a.iters), 2)
            row["write_jpegs_dev_optimized_ms"] = round(wall_ms(lambda: export.write_jpegs(dev, os.path.join(folder, "opt"), huffman="optimized"), a.iters), 2)
            row["write_pngs_dev_ms"] = round(wall_ms(lambda: export.write_pngs(dev, os.path.join(folder, "png")), a.iters), 2)
            pil_ms, pil_paths = pillow_save(host, folder, a.iters)
            same = all(open(p, "rb").read() == open(q, "rb").read() for p, q in zip(paths, pil_paths))
            st, crossing = stages(dev, folder, a.iters)
            png_bytes = sum(os.path.getsize(os.path.join(folder, "png", f"{i}.png")) for i in range(n))
            row.update(pillow_ms=round(pil_ms, 2), files_equal_pillows=bool(same), stages=st,
                       bytes=dict(jpeg=sum(os.path.getsize(p) for p in paths),
                                  jpeg_optimized=sum(os.path.getsize(os.path.join(folder, "opt", f"im_{i}.jpg")) for i in range(n)),
                                  pillow_jpeg=sum(os.path.getsize(p) for p in pil_paths), png=png_bytes,
                                  jpeg_to_host=crossing,
                                  png_to_host=int(png_bytes - n * 57 + n * _lib.load().tt_png_stripes(h, w, 3) * 1152)),
                       faster_than_pillow=dict(host=bool(row["write_jpegs_host_ms"] < pil_ms), dev=bool(row["write_jpegs_dev_ms"] < pil_ms)))
        rows.append(row)
    import PIL
    res = dict(tool="jpeg_export_bench", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), pillow=PIL.__version__,
               iters=a.iters, inputs="the generator of tests/png_reference.py, seeds 0 .. 13; quality 75, 4:2:0, standard tables", rows=rows,
               says="a record, not a gate; medians of --iters in one process after a warm-up; Pillow (libjpeg-turbo) runs on this machine's CPU, "
                    "one thread; kernel times are device events, the rest the host clock; files go to a temporary folder; png_to_host is the "
                    "files' streams plus 1152 bytes of counts per stripe")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

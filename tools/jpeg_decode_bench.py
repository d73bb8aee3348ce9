#!/usr/bin/env python
"""ingest.decode_jpeg timed against Pillow's per-frame ``open`` + ``load`` + upload (libjpeg-turbo, SIMD, one thread): 14 frames of
256 x 384 and of 576 x 1024 from the generator of tests/png_reference.py written by export.write_jpegs at quality 75 and 95 (4:2:0, the
standard tables), and the 640 x 480 fixture tests/golden/bridge_task1_im_0.jpg, 14 times over.

  pillow_ms        Image.open(BytesIO(bytes)) + load + np.asarray for every frame, one stack, one upload (median of --iters, wall clock)
  decode_jpeg_ms   ingest.decode_jpeg from the same file bytes to device pixels, status readback included (median of --iters, wall clock)
  stages           host_parse_ms (headers and decode tables, host clock); entropy_us (unstuffing, the entropy decoder, the DC sums) and
                   pixels_us: device events around ops.jpeg_entropy / ops.jpeg_pixels
  passes           --passes: the passes every sequence of frame 0 takes, from the CPU emulation of the scheme (tests/jpeg_decode_reference.py)
                   at the library's S and lane count: the kernel runs the same passes but does not report them.  The sequences of a frame
                   are walked in order by one workgroup, so there are no passes across sequences.
  equal            the decoded pixels equal Pillow's
  subsequence_alternatives   --variant S=PATH (repeatable): the same rows' entropy_us and decode_jpeg_ms with a library built with
                   -DTT_JPEG_SUBSEQ_BITS=S (`make variant NAME=s512 DEFS=-DTT_JPEG_SUBSEQ_BITS=512`), each in a child process of its own
                   that loads it through TT_LIBTTVDM

  --restart-rows N  every input twice in ONE process: written without markers and with ``restart_rows=N`` (the fixture's pixels are
                   re-encoded once for it, quality 75, 4:2:0): entropy_us and decode_jpeg_ms of both next to Pillow's time on the same
                   files, and ``sooner``: whether the marked files' time is below the marker-less files' of the same run.  The result
                   goes under "decode" of profiles/jpeg_restart_bench.json (tools/jpeg_export_bench.py fills "encode").

  --progressive     Pillow's ``progressive=True`` files (quality 75, 4:2:0) of 14 generator frames at 256 x 384 and at 576 x 1024 and of
                   the 640 x 480 fixture's pixels, once: the whole ``decode_jpeg(files, progressive=True)`` from the files' bytes against
                   Pillow on the same bytes; entropy_us (every round) and first_scans_us (the same call with the refinement scans' items
                   masked out: their rounds are launched and return at once) by device events, refine_us their difference: the
                   refinement rounds on their own.  The result goes to profiles/jpeg_progressive_bench.json.

The last row is ONE file, a request's image: without markers one workgroup decodes it, the case in which the scheme has the least to offer.

A record, not a gate.  Prints one JSON line and writes it to --out (default profiles/jpeg_decode_bench.json)."""
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


def pillow_decode(files):
    from PIL import Image
    frames = []
    for d in files:
        im = Image.open(io.BytesIO(d))
        im.load()
        frames.append(np.asarray(im))
    return torch.from_numpy(np.stack(frames)).cuda()


def restart_row(name, plain_files, marked_files, iters):
    """the same frames without and with restart markers: the decoder's device stage and the whole call, next to Pillow's"""
    from this_and_that_vdm_amd import _lib, ingest, ops

    def measure(files):
        heads = [ingest.parse_jpeg(d) for d in files]
        h0 = heads[0]
        shape = (h0.height, h0.width, h0.channels)
        sets = torch.from_numpy(np.stack([ingest.jpeg_decode_set([(h0.bits[k], h0.huffval[k]) for k in range(4)], h0.dc_table, h0.ac_table)]).view(np.int32)).cuda()
        blocks = _lib.load().tt_jpeg_blocks(*shape, ops.JPEG_SUBSAMPLING[h0.subsampling])
        per = h0.restart_interval * 6 if len(h0.spans) > 1 else blocks                  # 4:2:0 RGB: 6 blocks an MCU
        rows, base = [], 0
        for i, (d, h) in enumerate(zip(files, heads)):
            rows += [(base + o, n, i, k * per, min(per, blocks - k * per)) for k, (o, n) in enumerate(h.spans.tolist())]
            base += len(d)
        rows = np.array(rows, dtype=np.int64)
        scans = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).cuda()
        offs = torch.from_numpy(rows[:, 0].copy()).cuda()
        cols = [torch.from_numpy(rows[:, c].astype(np.int32)).cuda() for c in range(1, 5)]
        if len(rows) == len(files):                                                     # no markers: the per-frame entry point, as decode_jpeg takes it
            entropy = lambda: ops.jpeg_entropy(scans, offs, cols[0], int(rows[:, 1].max()), shape, h0.subsampling, sets)
        else:
            entropy = lambda: ops.jpeg_entropy_spans(scans, offs, *cols, int(rows[:, 1].max()), len(files), shape, h0.subsampling, sets)
        got = ingest.decode_jpeg(files, "cuda")
        return dict(file_bytes=int(sum(len(d) for d in files)), spans=int(len(rows)), restart_interval=int(h0.restart_interval),
                    equal=bool(torch.equal(got, pillow_decode(files))) and not bool(entropy()[1].any()),
                    entropy_us=round(events_us(entropy, iters), 1), decode_jpeg_ms=round(wall_ms(lambda: ingest.decode_jpeg(files, "cuda"), iters), 2),
                    pillow_ms=round(wall_ms(lambda: pillow_decode(files), iters), 2)), got

    plain, a = measure(plain_files)
    marked, b = measure(marked_files)
    return dict(input=name, frames=[len(plain_files), *a.shape[1:]], same_pixels=bool(torch.equal(a, b)), plain=plain, marked=marked,
                sooner=dict(entropy=bool(marked["entropy_us"] < plain["entropy_us"]), decode_jpeg=bool(marked["decode_jpeg_ms"] < plain["decode_jpeg_ms"])),
                marked_faster_than_pillow=bool(marked["decode_jpeg_ms"] < marked["pillow_ms"]))


def restart_main(a):
    """--restart-rows: the rows of the issue's table -> profiles/jpeg_restart_bench.json, key "decode" """
    from tests import png_reference as ref
    from this_and_that_vdm_amd import export
    rows = []
    for n, h, w in [(14, 256, 384), (14, 576, 1024)]:
        dev = torch.from_numpy(np.stack([ref.generator_frame(h, w, f) for f in range(n)], 0)).cuda()
        for quality in (75, 95):
            rows.append(restart_row(f"write_jpegs {h}x{w} quality {quality}", export.encode_jpeg(dev, quality=quality),
                                    export.encode_jpeg(dev, quality=quality, restart_rows=a.restart_rows), a.iters))
    with open(os.path.join(REPO, "tests", "golden", "bridge_task1_im_0.jpg"), "rb") as fh:
        pixels = pillow_decode([fh.read()])
    rows.append(restart_row("fixture bridge_task1_im_0.jpg's pixels re-encoded at quality 75 x 1 (a request's image)", export.encode_jpeg(pixels, quality=75),
                            export.encode_jpeg(pixels, quality=75, restart_rows=a.restart_rows), a.iters))
    import PIL
    res = dict(tool="jpeg_decode_bench --restart-rows", restart_rows=a.restart_rows, device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(),
               pillow=PIL.__version__, iters=a.iters, rows=rows,
               says="a record, not a gate; medians of --iters in one process after a warm-up; `plain` and `marked` are the same frames written without and "
                    "with restart markers; entropy_us is unstuffing + entropy decode + DC sums by device events, decode_jpeg_ms the whole call by the host "
                    "clock; Pillow (libjpeg-turbo) runs on this machine's CPU, one thread, and its time includes the upload of the raw pixels")
    merge_out(a.out, "decode", res)
    print(json.dumps(res))


def merge_out(path, key, res):
    """profiles/jpeg_restart_bench.json holds the decoder's and the encoder's record side by side: replace one, keep the other"""
    both = {}
    if os.path.exists(path):
        with open(path) as f:
            both = json.load(f)
    both[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(both, f, indent=1)
        f.write("\n")


def progressive_row(name, files, iters):
    from this_and_that_vdm_amd import ingest, ops
    heads = [ingest.parse_jpeg_progressive(d) for d in files]
    h0 = heads[0]
    shape = (h0.height, h0.width, h0.channels)
    blob, offs, lens, desc, tables = ingest._progressive_items(heads, files, list(range(len(files))))
    first = desc.copy()
    first[desc[:, 3] != 0] = 0                                                               # the refinement scans' items masked out
    dev = lambda x: torch.from_numpy(x).cuda()
    d_blob, d_offs, d_lens, d_desc, d_first, d_tables = dev(blob), dev(offs), dev(lens), dev(desc), dev(first), dev(tables.view(np.int32))
    entropy = lambda which: ops.jpeg_entropy_progressive(d_blob, d_offs, d_lens, which, d_tables, int(lens.max()), len(files), shape, h0.subsampling)
    coeffs, status = entropy(d_desc)
    quant = dev(h0.quant[None])
    got = ingest.decode_jpeg(files, "cuda", progressive=True)
    row = dict(input=name, frames=[len(files), *shape], file_bytes=int(sum(len(d) for d in files)), raw_bytes=int(got.numel()), scans=len(h0.scans),
               refinement_scans=int(sum(1 for s in h0.scans if s.ah)), longest_scan_bytes=int(lens.max()),
               equal=bool(torch.equal(got, pillow_decode(files))) and not bool(status.any()),
               pillow_ms=round(wall_ms(lambda: pillow_decode(files), iters), 2),
               decode_jpeg_ms=round(wall_ms(lambda: ingest.decode_jpeg(files, "cuda", progressive=True), iters), 2),
               stages=dict(host_parse_ms=round(wall_ms(lambda: ingest._progressive_items([ingest.parse_jpeg_progressive(d) for d in files], files,
                                                                                        list(range(len(files)))), iters), 3),
                           entropy_us=round(events_us(lambda: entropy(d_desc), iters), 1), first_scans_us=round(events_us(lambda: entropy(d_first), iters), 1),
                           pixels_us=round(events_us(lambda: ops.jpeg_pixels(coeffs, shape, h0.subsampling, quant), iters), 1)))
    row["stages"]["refine_us"] = round(row["stages"]["entropy_us"] - row["stages"]["first_scans_us"], 1)
    row["faster_than_pillow"] = bool(row["decode_jpeg_ms"] < row["pillow_ms"])
    return row


def progressive_main(a):
    """--progressive: the rows of the issue -> profiles/jpeg_progressive_bench.json"""
    from PIL import Image
    from tests import png_reference as ref

    def save(frame):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="JPEG", quality=75, subsampling=2, progressive=True)
        return buf.getvalue()
    rows = [progressive_row(f"Pillow progressive {h}x{w} quality 75 4:2:0 x {n}", [save(ref.generator_frame(h, w, f)) for f in range(n)], a.iters)
            for n, h, w in [(14, 256, 384), (14, 576, 1024)]]
    with Image.open(os.path.join(REPO, "tests", "golden", "bridge_task1_im_0.jpg")) as im:
        pixels = np.asarray(im.convert("RGB"))
    rows.append(progressive_row("fixture bridge_task1_im_0.jpg's pixels as a progressive file x 1 (a request's image)", [save(pixels)], a.iters))
    import PIL
    res = dict(tool="jpeg_decode_bench --progressive", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), pillow=PIL.__version__,
               iters=a.iters, rows=rows,
               says="a record, not a gate; medians of --iters in one process after a warm-up; decode_jpeg_ms is the whole call from the files' bytes by the "
                    "host clock, status readback included; entropy_us is unstuffing + every round by device events, first_scans_us the same call with the "
                    "refinement scans' items masked out, refine_us their difference; Pillow (libjpeg-turbo) runs on this machine's CPU, one thread, and "
                    "its time includes the upload of the raw pixels")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def row_of(name, files, iters, passes):
    from tests import jpeg_decode_reference as dec
    from this_and_that_vdm_amd import _lib, ingest, ops
    heads = [ingest.parse_jpeg(d) for d in files]
    h0 = heads[0]
    shape = (h0.height, h0.width, h0.channels)

    def host():
        hs = [ingest.parse_jpeg(d) for d in files]
        return [ingest.jpeg_decode_set([(h.bits[k], h.huffval[k]) for k in range(4)], h.dc_table, h.ac_table) for h in hs[:1]]
    sets = torch.from_numpy(np.stack(host()).view(np.int32)).cuda()
    blobs = [d[h.scan_offset:h.scan_offset + h.scan_bytes] for d, h in zip(files, heads)]
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    scans = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
    dlens = torch.from_numpy(lens.astype(np.int32)).cuda()
    quant = torch.from_numpy(h0.quant[None]).cuda()
    coeffs, status = ops.jpeg_entropy(scans, offs, dlens, int(lens.max()), shape, h0.subsampling, sets)
    got = ingest.decode_jpeg(files, "cuda")
    row = dict(input=name, frames=[len(files), *shape], file_bytes=int(sum(len(d) for d in files)), raw_bytes=int(got.numel()),
               plain_bits_frame0=8 * len(dec.unstuff(blobs[0])[0]), sequence_bits=int(_lib.load().tt_jpeg_sequence_bits()),
               equal=bool(torch.equal(got, pillow_decode(files))) and not bool(status.any()),
               pillow_ms=round(wall_ms(lambda: pillow_decode(files), iters), 2),
               decode_jpeg_ms=round(wall_ms(lambda: ingest.decode_jpeg(files, "cuda"), iters), 2),
               stages=dict(host_parse_ms=round(wall_ms(host, iters), 3),
                           entropy_us=round(events_us(lambda: ops.jpeg_entropy(scans, offs, dlens, int(lens.max()), shape, h0.subsampling, sets), iters), 1),
                           pixels_us=round(events_us(lambda: ops.jpeg_pixels(coeffs, shape, h0.subsampling, quant), iters), 1)))
    row["faster_than_pillow"] = bool(row["decode_jpeg_ms"] < row["pillow_ms"])
    if passes:
        hd = dec.parse(files[0])
        S = row["sequence_bits"] // 256
        row["passes_frame0"] = dec.entropy_lanes(hd["scan"], dec.decode_set(hd), hd["dc"], hd["ac"], *shape, dec.S420 if h0.subsampling == "4:2:0" else dec.S444, S, 256)[2]
    else:
        row["passes_frame0"] = "not measured"
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--passes", action="store_true", help="count frame 0's passes with the CPU emulation (slow: minutes for the large frames)")
    ap.add_argument("--variant", action="append", default=[], metavar="S=PATH", help="a library built with another TT_JPEG_SUBSEQ_BITS")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--restart-rows", type=int, default=0, metavar="N", help="compare files written with restart_rows=N against the marker-less ones")
    ap.add_argument("--progressive", action="store_true", help="Pillow's progressive files through decode_jpeg(progressive=True)")
    ap.add_argument("--out", default=None, help="default profiles/jpeg_decode_bench.json; with --restart-rows profiles/jpeg_restart_bench.json; with "
                                                "--progressive profiles/jpeg_progressive_bench.json")
    a = ap.parse_args()
    a.out = a.out or os.path.join(REPO, "profiles", "jpeg_progressive_bench.json" if a.progressive else
                                  ("jpeg_restart_bench.json" if a.restart_rows else "jpeg_decode_bench.json"))
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench: needs a GPU (there is no CPU fallback)")
    if a.restart_rows:
        return restart_main(a)
    if a.progressive:
        return progressive_main(a)
    from tests import png_reference as ref
    from this_and_that_vdm_amd import export
    rows = []
    for n, h, w in [(14, 256, 384), (14, 576, 1024)]:
        dev = torch.from_numpy(np.stack([ref.generator_frame(h, w, f) for f in range(n)], 0)).cuda()
        for quality in (75, 95):
            rows.append(row_of(f"write_jpegs {h}x{w} quality {quality}", export.encode_jpeg(dev, quality=quality), a.iters, a.passes))
    with open(os.path.join(REPO, "tests", "golden", "bridge_task1_im_0.jpg"), "rb") as fh:
        fixture = fh.read()
    rows.append(row_of("fixture bridge_task1_im_0.jpg x 14", [fixture] * 14, a.iters, a.passes))
    rows.append(row_of("fixture bridge_task1_im_0.jpg x 1 (a request's image)", [fixture], a.iters, a.passes))
    if a.child:
        print(json.dumps([dict(input=r["input"], subsequence_bits=r["sequence_bits"] // 256, equal=r["equal"], entropy_us=r["stages"]["entropy_us"],
                               decode_jpeg_ms=r["decode_jpeg_ms"]) for r in rows]))
        return
    alternatives = {}
    for spec in a.variant:
        import subprocess
        name, path = spec.split("=", 1)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)], env=dict(os.environ, TT_LIBTTVDM=os.path.abspath(path)),
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"jpeg_decode_bench: the variant {spec} failed:\n{r.stderr[-2000:]}")
        alternatives[name] = json.loads(r.stdout.splitlines()[-1])
        assert all(row["subsequence_bits"] == int(name) for row in alternatives[name]), (spec, alternatives[name][0])
    import PIL
    res = dict(tool="jpeg_decode_bench", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), pillow=PIL.__version__, iters=a.iters,
               subsequence_bits=rows[0]["sequence_bits"] // 256, rows=rows,
               subsequence_alternatives=alternatives or "not measured",
               says="a record, not a gate; medians of --iters in one process after a warm-up; Pillow (libjpeg-turbo) runs on this machine's CPU, one "
                    "thread, and its time includes the upload of the raw pixels; kernel times are device events, the rest the host clock")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

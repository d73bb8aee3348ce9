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

The last row is ONE file, a request's image: one workgroup decodes it, the case in which the scheme has the least to offer.

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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench: needs a GPU (there is no CPU fallback)")
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

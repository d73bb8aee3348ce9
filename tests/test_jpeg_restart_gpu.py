"""GPU: restart intervals in the JPEG export and import (include/ttvdm.h: "JPEG export" rule 6a, "JPEG import" rules 1a and 4a).
``export.encode_jpeg(..., restart_interval / restart_rows)`` against Pillow's ``restart_marker_blocks`` / ``restart_marker_rows`` byte
for byte, from host and device frames, with standard and optimized tables; ``ingest.decode_jpeg`` against Pillow's pixels on Pillow's
files and on the export's own, in batches of one and of several intervals; a corrupt frame between two good ones, through the parser
and through the status word; spans longer than one sequence of the entropy decoder; poison behind every buffer and the scan bound on
noise with a marker behind every MCU; the round trips through ``write_jpegs`` / ``read_jpegs`` and ``write_mjpeg`` / ``read_mjpeg_video``.

Nothing here is a tolerance: equality is the bound.  The shapes, intervals and qualities are those of tests/test_jpeg_restart_cpu.py,
where the restatement itself is held to Pillow."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_decode_reference as dec
from tests import jpeg_reference as ref
from tests import jpeg_restart_reference as rr
from tests.test_jpeg_restart_cpu import QUALITIES, SHAPE_IDS, SHAPES, STUFFED, STUFFED_PATTERN, intervals_of, library_tables, pillow_file, pillow_pixels
from this_and_that_vdm_amd import _lib, export, ingest, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUB_NAMES = {0: "4:4:4", 2: "4:2:0"}
POISON, TAIL = 0xA5, 4096


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _frames(h, w, ch):
    return np.stack([ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch)], 0)


@functools.lru_cache(maxsize=None)
def _pillow_files(shape, quality, ri_index):
    """Pillow's files of _frames(shape) at one of intervals_of(shape): computed once, shared by the encoder and the decoder tests"""
    h, w, ch, sub = shape
    ri, kw = intervals_of(h, w, ch, sub)[ri_index]
    return ri, kw, [pillow_file(f, quality, sub, **kw) for f in _frames(h, w, ch)]


# ---- the encoder
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_encode_jpeg_with_restart_intervals_equals_pillows_files(shape):
    h, w, ch, sub = shape
    frames = _frames(h, w, ch)
    x = _dev(frames)
    for quality in QUALITIES:
        for k in range(6):
            ri, kw, want = _pillow_files(shape, quality, k)
            ours = dict(restart_rows=kw["restart_marker_rows"]) if "restart_marker_rows" in kw else dict(restart_interval=ri)
            got = export.encode_jpeg(x, quality=quality, subsampling=SUB_NAMES[sub], **ours)
            assert got == want, (quality, ri, [len(d) for d in got], [len(d) for d in want])
            if "restart_marker_rows" in kw:                                                              # rows are MCUs per row: the same file either way
                assert export.encode_jpeg(x, quality=quality, subsampling=SUB_NAMES[sub], restart_interval=ri) == want
    ri, kw, want = _pillow_files(shape, 75, 1)
    assert export.encode_jpeg(frames, quality=75, subsampling=SUB_NAMES[sub], restart_interval=ri) == want                # host frames
    assert export.encode_jpeg(x, quality=75, subsampling=SUB_NAMES[sub], restart_interval=ri) == want                     # ... and again: the same bytes


def test_no_interval_is_todays_file():
    frames = _frames(40, 56, 3)
    today = export.encode_jpeg(_dev(frames), quality=90)
    assert today == [ref.jpeg_file(f, 90, ref.S420) for f in frames]
    assert export.encode_jpeg(_dev(frames), quality=90, restart_interval=0, restart_rows=0) == today
    coeffs, counts = ops.jpeg_coeffs(_dev(frames), 90, "4:2:0")
    assert torch.equal(ops.jpeg_counts_restart(coeffs, (40, 56, 3), "4:2:0", 0), counts)


def test_the_stuffed_byte_before_a_marker():
    want = rr.jpeg_file(STUFFED["frame"], STUFFED["quality"], STUFFED["sub"], STUFFED["ri"])
    assert STUFFED_PATTERN.search(want)
    got = export.encode_jpeg(_dev(STUFFED["frame"][None]), quality=STUFFED["quality"], subsampling=SUB_NAMES[STUFFED["sub"]], restart_interval=STUFFED["ri"])
    assert got == [want]
    assert np.array_equal(ingest.decode_jpeg(got, DEV).cpu().numpy()[0], pillow_pixels(want))


@pytest.mark.parametrize("shape,ri", [((40, 56, 3, 2), 4), ((33, 17, 3, 0), 1), ((24, 40, 1, 0), 7), ((48, 48, 3, 0), 2)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_optimized_tables_count_with_the_predictor_resets(shape, ri):
    h, w, ch, sub = shape
    frames = _frames(h, w, ch)
    got = export.encode_jpeg(_dev(frames), quality=75, subsampling=SUB_NAMES[sub], huffman="optimized", restart_interval=ri)
    for i in range(2):
        want = rr.jpeg_file(frames[i], 75, sub, ri, tables=library_tables)
        assert got[i] == want, i
        assert np.array_equal(pillow_pixels(got[i]), rr.decode(want)[0]), i
    bpm = rr.blocks_per_mcu(ch, sub)
    coeffs, _ = ops.jpeg_coeffs(_dev(frames), 75, SUB_NAMES[sub], counts=False)
    counts = ops.jpeg_counts_restart(coeffs, (h, w, ch), SUB_NAMES[sub], ri).cpu().numpy().view(np.uint32).astype(np.int64)
    for i in range(2):
        coefs, comps, _ = ref.coefficients(frames[i], 75, sub)
        assert np.array_equal(counts[i], rr.symbol_counts(coefs, comps, ri * bpm)), i


# ---- the decoder
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_decode_jpeg_of_pillows_restart_files_equals_pillows_pixels(shape):
    h, w, ch, sub = shape
    for quality in QUALITIES:
        for k in range(6):
            ri, _, files = _pillow_files(shape, quality, k)
            want = np.stack([pillow_pixels(d) for d in files])
            got = ingest.decode_jpeg(files, DEV)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, ch)
            assert np.array_equal(got.cpu().numpy(), want), (quality, ri, np.argwhere(got.cpu().numpy() != want)[:5])
    # files of several intervals, and of none, in one call: supported; every frame is as on its own
    mixed = [_pillow_files(shape, 75, k)[2][k & 1] for k in range(6)] + [pillow_file(_frames(h, w, ch)[1], 75, sub)]
    assert len({ingest.parse_jpeg(d).restart_interval for d in mixed}) >= 4
    got = ingest.decode_jpeg(mixed, DEV).cpu().numpy()
    assert np.array_equal(got, np.stack([pillow_pixels(d) for d in mixed]))
    # ... and the export's own files, optimized tables among them
    own = export.encode_jpeg(_dev(_frames(h, w, ch)), quality=92, subsampling=SUB_NAMES[sub], restart_rows=1) + \
        export.encode_jpeg(_dev(_frames(h, w, ch)), quality=60, subsampling=SUB_NAMES[sub], restart_interval=2, huffman="optimized")
    assert np.array_equal(ingest.decode_jpeg(own, DEV).cpu().numpy(), np.stack([pillow_pixels(d) for d in own]))


def _spans_raw(files):
    """what ingest.decode_jpeg does with marked files, on raw pointers with poison behind every buffer (a file of one span goes through
    tt_jpeg_entropy_spans here too) -> (pixels [n, h, w, ch], status [n])"""
    lib = _lib.load()
    heads = [ingest.parse_jpeg(d) for d in files]
    h0 = heads[0]
    h, w, ch, sub = h0.height, h0.width, h0.channels, ops.JPEG_SUBSAMPLING[h0.subsampling]
    n, blocks, bpm = len(files), lib.tt_jpeg_blocks(h, w, ch, sub), rr.blocks_per_mcu(ch, sub)
    pad = [0] * (3 - ch)
    sets = np.stack([ingest.jpeg_decode_set([(hd.bits[k], hd.huffval[k]) for k in range(4)], hd.dc_table + pad, hd.ac_table + pad) for hd in heads])
    blob = np.frombuffer(b"".join(files), dtype=np.uint8).copy()                                        # whole files: the spans' offsets are the parser's
    rows, base = [], 0
    for i, (d, hd) in enumerate(zip(files, heads)):
        per = hd.restart_interval * bpm if len(hd.spans) > 1 else blocks
        rows += [(base + o, ln, i, k * per, min(per, blocks - k * per)) for k, (o, ln) in enumerate(hd.spans.tolist())]
        base += len(d)
    rows = np.array(rows, dtype=np.int64)
    s, max_bytes = len(rows), int(rows[:, 1].max())
    ws_bytes = lib.tt_jpeg_entropy_ws_bytes(s, max_bytes)
    src, coeffs, status, ws = (torch.full((nb + TAIL,), POISON, dtype=torch.uint8, device=DEV) for nb in (blob.size, n * blocks * 128, 4 * n, ws_bytes))
    src[:blob.size] = _dev(blob)
    cols = [_dev(rows[:, 0])] + [_dev(rows[:, c].astype(np.int32)) for c in range(1, 5)]                 # held until the synchronize below
    d_sets, d_quant = _dev(sets.view(np.int32)), _dev(np.stack([hd.quant for hd in heads]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tt_jpeg_entropy_spans(src.data_ptr(), blob.size, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), cols[4].data_ptr(),
                                         max_bytes, s, n, h, w, ch, sub, d_sets.data_ptr(), n, coeffs.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, stream),
               "tt_jpeg_entropy_spans")
    frames = torch.full((n * h * w * ch + TAIL,), POISON, dtype=torch.uint8, device=DEV)
    _lib.check(lib.tt_jpeg_pixels(coeffs.data_ptr(), n, h, w, ch, sub, d_quant.data_ptr(), n, frames.data_ptr(), stream), "tt_jpeg_pixels")
    torch.cuda.synchronize()
    for name, buf, used in (("scans", src, blob.size), ("coeffs", coeffs, n * blocks * 128), ("status", status, 4 * n), ("ws", ws, ws_bytes), ("frames", frames, n * h * w * ch)):
        assert bool((buf[used:] == POISON).all()), name
    return frames[:n * h * w * ch].view(n, h, w, ch).cpu().numpy(), status[:4 * n].cpu().numpy().view(np.int32)


def test_a_corrupt_frame_between_two_good_ones():
    h, w, ch, sub = 48, 48, 3, 0                                                                         # 36 MCUs
    frames = [ref.smooth_frame(h, w, 3), ref.noise_frame(h, w, 4), ref.smooth_frame(h, w, 5)]
    good = [pillow_file(f, 75, sub, restart_marker_blocks=7) for f in frames]                            # 5 markers
    spans = rr.parse(good[1])["spans"]
    marker = spans[2][0] + spans[2][1]
    renumbered = good[1][:marker + 1] + bytes([0xd6]) + good[1][marker + 2:]
    with pytest.raises(ValueError, match="decode_jpeg: file 1: tt_jpeg_parse_spans: .*is RST6 where RST2 is due"):
        ingest.decode_jpeg([good[0], renumbered, good[2]], DEV)
    deleted = good[1][:marker] + good[1][marker + 2:]
    with pytest.raises(ValueError, match="decode_jpeg: file 1: tt_jpeg_parse_spans: .*is RST3 where RST2 is due"):
        ingest.decode_jpeg([good[0], deleted, good[2]], DEV)
    last = spans[4][0] + spans[4][1]
    with pytest.raises(ValueError, match="decode_jpeg: file 1: tt_jpeg_parse_spans: 4 restart markers where"):
        ingest.decode_jpeg([good[0], good[1][:last] + good[1][last + 2:], good[2]], DEV)
    # a file the parser has no quarrel with: DRI says 6 where the scan was written with 7 -- 5 markers either way -- so every span holds
    # a block count other than its place has room for: the status word of ITS frame, and the neighbours decode
    at = good[1].index(b"\xff\xdd\x00\x04\x00\x07")
    wrong = good[1][:at + 5] + b"\x06" + good[1][at + 6:]
    assert rr.decode(wrong)[1] & dec.BLOCKS
    with pytest.raises(ValueError, match="decode_jpeg: frame 1 is corrupt or truncated .*the wrong number of blocks"):
        ingest.decode_jpeg([good[0], wrong, good[2]], DEV)
    pixels, status = _spans_raw([good[0], wrong, good[2]])
    assert status[0] == 0 and status[2] == 0 and status[1] & 4
    assert np.array_equal(pixels[0], pillow_pixels(good[0])) and np.array_equal(pixels[2], pillow_pixels(good[2]))


def test_spans_longer_than_one_sequence():
    frame = ref.noise_frame(128, 192, 2)                                                                 # 384 MCUs in 4:4:4
    one = pillow_file(frame, 100, 0, restart_marker_blocks=1000)
    two = pillow_file(frame, 100, 0, restart_marker_blocks=192)
    seq = _lib.load().tt_jpeg_sequence_bits()
    for data, count in ((one, 1), (two, 2)):
        spans = rr.parse(data)["spans"]
        assert len(spans) == count
        for at, n in spans:
            assert 8 * len(dec.unstuff(data[at:at + n])[0]) > seq                                        # the true state is carried from a sequence to the next
        want = pillow_pixels(data)
        assert np.array_equal(ingest.decode_jpeg([data], DEV).cpu().numpy()[0], want)
        pixels, status = _spans_raw([data, data])                                                       # the one span too through the spans' entry point
        assert status.tolist() == [0, 0] and np.array_equal(pixels[0], want) and np.array_equal(pixels[1], want)
    assert export.encode_jpeg(_dev(frame[None]), quality=100, subsampling="4:4:4", restart_interval=192) == [two]


@pytest.mark.parametrize("shape", [(33, 17, 3, 2), (40, 56, 3, 0), (24, 40, 1, 0)], ids=lambda s: "x".join(map(str, s)))
def test_poison_behind_the_decoders_buffers_stays(shape):
    for k in (0, 2, 3):
        _, _, files = _pillow_files(shape, 92, k)
        pixels, status = _spans_raw(files)
        assert status.tolist() == [0, 0] and np.array_equal(pixels, np.stack([pillow_pixels(d) for d in files]))


@pytest.mark.parametrize("frame,sub,quality,ri", [(ref.noise_frame(128, 192, 2), 0, 100, 1), (ref.noise_frame(128, 192, 2), 2, 100, 5), (STUFFED["frame"], 0, 90, 1),
                                                  (ref.noise_frame(33, 17, 2), 2, 92, 1)], ids=["noise-444-ri1", "noise-420-ri5", "stuffed-pad", "33x17-420-ri1"])
def test_poison_behind_the_encoders_buffers_stays_and_the_bound_holds(frame, sub, quality, ri):
    lib = _lib.load()
    h, w, ch = frame.shape
    n = 2
    frames = np.stack([frame, frame[::-1]], 0)
    blocks, stride, ws_bytes = lib.tt_jpeg_blocks(h, w, ch, sub), lib.tt_jpeg_scan_bound_restart(h, w, ch, sub, ri), lib.tt_jpeg_scan_restart_ws_bytes(n, h, w, ch, sub, ri)
    assert stride > lib.tt_jpeg_scan_bound(h, w, ch, sub) and ws_bytes > lib.tt_jpeg_scan_ws_bytes(n, h, w, ch, sub)

    def poisoned(nbytes):
        return torch.full((nbytes + TAIL,), POISON, dtype=torch.uint8, device=DEV)

    x = _dev(frames)
    coeffs, counts, out, lengths, ws = poisoned(n * blocks * 128), poisoned(n * 4096), poisoned(n * stride), poisoned(4 * n), poisoned(ws_bytes)
    tables = _dev(np.stack([t.codes for t in export.jpeg_standard_tables()]).view(np.int32)[None])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tt_jpeg_coeffs(x.data_ptr(), n, h, w, ch, quality, sub, coeffs.data_ptr(), None, stream), "tt_jpeg_coeffs")
    _lib.check(lib.tt_jpeg_counts_restart(coeffs.data_ptr(), n, h, w, ch, sub, ri, counts.data_ptr(), stream), "tt_jpeg_counts_restart")
    _lib.check(lib.tt_jpeg_scan_restart(coeffs.data_ptr(), n, h, w, ch, sub, ri, tables.data_ptr(), 1, out.data_ptr(), n * stride, lengths.data_ptr(), ws.data_ptr(),
                                        ws_bytes, stream), "tt_jpeg_scan_restart")
    torch.cuda.synchronize()
    for name, buf, used in (("coeffs", coeffs, n * blocks * 128), ("counts", counts, n * 4096), ("out", out, n * stride), ("lengths", lengths, 4 * n), ("ws", ws, ws_bytes)):
        assert bool((buf[used:] == POISON).all()), name
    got_len, host = lengths[:4 * n].cpu().numpy().view(np.int32), out.cpu().numpy()
    bpm = rr.blocks_per_mcu(ch, sub)
    for i in range(n):
        coefs, comps, _ = ref.coefficients(frames[i], quality, sub)
        want = rr.scan_bytes(coefs, comps, ri * bpm)
        assert int(got_len[i]) == len(want) <= stride, (i, int(got_len[i]), len(want), stride)
        assert host[i * stride:i * stride + got_len[i]].tobytes() == want, i
        assert (host[i * stride + got_len[i]:(i + 1) * stride] == POISON).all()                         # nothing at or beyond the length is written
        assert np.array_equal(counts[i * 4096:(i + 1) * 4096].cpu().numpy().view(np.uint32).reshape(4, 256), rr.symbol_counts(coefs, comps, ri * bpm)), i


# ---- the paths it is for
def test_the_round_trips_give_the_marker_less_routes_pixels(tmp_path):
    frames = _dev(np.stack([ref.smooth_frame(40, 72, s) for s in range(3)] + [ref.noise_frame(40, 72, 9)], 0))
    export.write_jpegs(frames, str(tmp_path / "plain"), quality=90)
    plain = ingest.read_jpegs(str(tmp_path / "plain"), device=DEV)
    paths = export.write_jpegs(frames, str(tmp_path / "marked"), quality=90, restart_rows=1)
    with open(paths[0], "rb") as fh:
        hd = ingest.parse_jpeg(fh.read())
    assert hd.restart_interval == 5 and len(hd.spans) == 3                                               # 72 / 16 -> 5 MCUs a row, 3 rows
    marked = ingest.read_jpegs(str(tmp_path / "marked"), device=DEV)
    assert torch.equal(marked, plain)
    assert np.array_equal(marked.cpu().numpy(), np.stack([pillow_pixels(open(p, "rb").read()) for p in paths]))
    a, b = metrics.compare_frames(marked, frames), metrics.compare_frames(plain, frames)
    assert np.array_equal(a.frame_mse, b.frame_mse) and np.array_equal(a.frame_ssim, b.frame_ssim) and float(np.min(a.frame_mse)) > 0.0
    export.write_mjpeg(frames, str(tmp_path / "marked.avi"), fps=4, quality=90, restart_rows=1)
    export.write_mjpeg(frames, str(tmp_path / "plain.avi"), fps=4, quality=90)
    assert all(ingest.parse_jpeg(d).restart_interval == 5 for d in export.read_mjpeg_frames(str(tmp_path / "marked.avi")))
    assert torch.equal(ingest.read_mjpeg_video(str(tmp_path / "marked.avi"), device=DEV), plain)
    assert torch.equal(ingest.read_mjpeg_video(str(tmp_path / "plain.avi"), device=DEV), plain)

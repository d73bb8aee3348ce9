"""GPU: the kernels of the JPEG import.  tt_jpeg_entropy as the exact inverse of tt_jpeg_scan on the export tests' shapes (standard and
optimized tables, one table set and one per frame); tt_jpeg_pixels against the restatement of tests/jpeg_decode_reference.py;
ingest.decode_jpeg of Pillow's files against ``np.asarray(Image.open(...))`` -- odd sizes, both subsamplings, grey, the qualities 1, 75
and 100, optimized tables, the 640 x 480 fixture --; a noise frame whose scan spans more than two sequences of the entropy decoder; a
stuffed FF 00 pair that straddles an unstuffing chunk; a scan cut short; frame independence; poison behind every buffer.

Nothing here is a tolerance: the format is integers from end to end, so equality is the bound.  (The restatement itself is held to
Pillow's decoder in tests/test_jpeg_decode_cpu.py.)"""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_reference as dec
from tests import jpeg_reference as ref
from this_and_that_vdm_amd import _lib, export, ingest, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUBS = {"4:4:4": ref.S444, "4:2:0": ref.S420}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bridge_task1_im_0.jpg")
POISON, TAIL = 0xA5, 4096

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _pillow(frame, quality, sub, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, **kw)
    return buf.getvalue()


def _pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


# ---- the library called with poison behind every buffer: what ingest.decode_jpeg does, on raw pointers
def _poisoned(nbytes):
    return torch.full((nbytes + TAIL,), POISON, dtype=torch.uint8, device=DEV)


def _entropy_raw(scans, shape, sub, sets, lengths=None):
    """scans: the frames' stuffed bytes; sets uint32 [1 or n, 1028] -> (coeffs int16 [n, blocks, 64], status [n]); asserts the poison"""
    lib = _lib.load()
    n, (h, w, ch) = len(scans), shape
    lens = np.array([len(s) for s in scans] if lengths is None else lengths, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])[:-1]]).astype(np.int64)
    blob = np.frombuffer(b"".join(scans), dtype=np.uint8)
    blocks, max_bytes = lib.tt_jpeg_blocks(h, w, ch, sub), int(lens.max())
    ws_bytes = lib.tt_jpeg_entropy_ws_bytes(n, max_bytes)
    src, coeffs, status, ws = _poisoned(blob.size), _poisoned(n * blocks * 128), _poisoned(4 * n), _poisoned(ws_bytes)
    src[:blob.size] = _dev(blob)
    d_offs, d_lens, d_sets = _dev(offs), _dev(lens.astype(np.uint32).view(np.int32)), _dev(sets.view(np.int32))      # held until the synchronize below
    _lib.check(lib.tt_jpeg_entropy(src.data_ptr(), blob.size, d_offs.data_ptr(), d_lens.data_ptr(), max_bytes, n, h, w, ch,
                                   sub, d_sets.data_ptr(), sets.shape[0], coeffs.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tt_jpeg_entropy")
    torch.cuda.synchronize()
    for name, buf, used in (("scans", src, blob.size), ("coeffs", coeffs, n * blocks * 128), ("status", status, 4 * n), ("ws", ws, ws_bytes)):
        assert bool((buf[used:] == POISON).all()), name
    return coeffs[:n * blocks * 128].view(torch.int16).view(n, blocks, 64), status[:4 * n].cpu().numpy().view(np.int32)


def _pixels_raw(coeffs, shape, sub, quant):
    lib = _lib.load()
    n, (h, w, ch) = coeffs.shape[0], shape
    frames = _poisoned(n * h * w * ch)
    d_quant = _dev(quant)
    _lib.check(lib.tt_jpeg_pixels(coeffs.data_ptr(), n, h, w, ch, sub, d_quant.data_ptr(), quant.shape[0], frames.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tt_jpeg_pixels")
    torch.cuda.synchronize()
    assert bool((frames[n * h * w * ch:] == POISON).all()), "frames"
    return frames[:n * h * w * ch].view(n, h, w, ch).cpu().numpy()


def _decode_raw(files):
    """-> (pixels uint8 [n, h, w, ch], status)"""
    heads = [ingest.parse_jpeg(d) for d in files]
    h0 = heads[0]
    pad = [0] * (3 - h0.channels)
    sets = np.stack([ingest.jpeg_decode_set([(h.bits[k], h.huffval[k]) for k in range(4)], h.dc_table + pad, h.ac_table + pad) for h in heads])
    shape, sub = (h0.height, h0.width, h0.channels), SUBS[h0.subsampling]
    coeffs, status = _entropy_raw([d[h.scan_offset:h.scan_offset + h.scan_bytes] for d, h in zip(files, heads)], shape, sub, sets)
    return _pixels_raw(coeffs, shape, sub, np.stack([h.quant for h in heads])), status


# ---- the exact inverse of tt_jpeg_scan, and the reconstruction of those coefficients
SHAPES = [(1, 1, 3), (8, 8, 3), (8, 24, 3), (24, 8, 3), (9, 17, 3), (17, 9, 3), (15, 33, 3), (37, 53, 3), (64, 96, 3), (9, 17, 1), (128, 192, 3),
          (24, 520, 3), (24, 520, 1)]                                                   # the shapes of tests/test_jpeg_export_gpu.py
EDGES = [(8, 9, 3), (18, 33, 3), (40, 41, 3), (50, 34, 3), (9, 3, 3), (9, 1, 3), (5, 4, 3)]   # where the upsampler's clamps and its narrow-plane rule show


@functools.lru_cache(maxsize=None)
def _frames(shape):
    h, w, ch = shape
    return np.stack([ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch)], 0)


def _component_quant(quality):
    q = export.jpeg_quant_tables(quality)
    return np.stack([q[0], q[1], q[1]])[None]


@pytest.mark.parametrize("quality", [1, 75, 100])
@pytest.mark.parametrize("sub", list(SUBS))
@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=_ids)
def test_entropy_inverts_scan_and_pixels_equal_the_restatement(shape, sub, quality):
    frames = _frames(shape)
    coeffs, counts = ops.jpeg_coeffs(_dev(frames), quality, sub)
    want = coeffs.cpu().numpy()
    standard = export.jpeg_standard_tables()
    cnt = counts.cpu().numpy().view(np.uint32)
    optimized = [[export.jpeg_optimized_table(cnt[i, k]) for k in range(4)] for i in range(2)]
    for per_frame in ([standard], optimized):                                        # ntables 1, and one set per frame
        codes = _dev(np.stack([np.stack([t.codes for t in ts]) for ts in per_frame]).view(np.int32))
        out, lengths = ops.jpeg_scan(coeffs, shape, sub, codes)
        lens = lengths.cpu().numpy()
        scans = [out[i, :int(lens[i])].cpu().numpy().tobytes() for i in range(2)]
        got, status = _entropy_raw(scans, shape, SUBS[sub], np.stack([ingest.jpeg_decode_set(ts) for ts in per_frame]))
        assert status.tolist() == [0, 0]
        got = got.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # ops.jpeg_entropy reads jpeg_scan's own rows in place
    offsets = torch.arange(2, device=DEV, dtype=torch.int64) * out.shape[1]
    again, status = ops.jpeg_entropy(out, offsets, lengths, int(lens.max()), shape, sub, _dev(np.stack([ingest.jpeg_decode_set(ts) for ts in optimized]).view(np.int32)))
    assert torch.equal(again, coeffs) and status.cpu().tolist() == [0, 0]
    quant = _component_quant(quality)
    pixels = _pixels_raw(coeffs, shape, SUBS[sub], quant)
    for i in range(2):
        assert np.array_equal(pixels[i], dec.pixels(want[i], quant[0], *shape, SUBS[sub])), i
    assert np.array_equal(ops.jpeg_pixels(coeffs, shape, sub, _dev(quant)).cpu().numpy(), pixels)


# ---- decode_jpeg against Pillow
SIZES = [(1, 1), (8, 8), (8, 24), (24, 8), (8, 9), (9, 17), (17, 9), (18, 33), (40, 41), (50, 34), (37, 53), (64, 96)]


@pytest.mark.parametrize("kind", ["4:4:4", "4:2:0", "grey"])
@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_decode_jpeg_of_pillows_files_equals_pillows_pixels(size, kind):
    h, w = size
    ch, sub = (1, 0) if kind == "grey" else (3, SUBS[kind])
    for quality in (1, 75, 100):
        frames = [ref.smooth_frame(h, w, 3, ch), ref.noise_frame(h, w, 4, ch), ref.checker_frame(h, w, ch)]
        files = [_pillow(f, quality, sub, optimize=(i == 1)) for i, f in enumerate(frames)]
        want = np.stack([_pillow_pixels(d) for d in files])
        got = ingest.decode_jpeg(files, DEV)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, h, w, ch) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), (quality, np.argwhere(got.cpu().numpy() != want)[:5])
        raw, status = _decode_raw(files)
        assert status.tolist() == [0, 0, 0] and np.array_equal(raw, want)


def test_the_fixture_decodes_as_in_pillow():
    with open(FIXTURE, "rb") as fh:
        data = fh.read()
    want = _pillow_pixels(data)
    assert want.shape == (480, 640, 3)
    assert np.array_equal(ingest.decode_jpeg(FIXTURE, DEV).cpu().numpy()[0], want)
    raw, status = _decode_raw([data, data])
    assert status.tolist() == [0, 0] and np.array_equal(raw[0], want) and np.array_equal(raw[1], want)


def test_frames_of_one_call_are_independent_and_carry_their_own_tables():
    frames = [ref.smooth_frame(37, 53, 1), ref.noise_frame(37, 53, 2), ref.checker_frame(37, 53)]
    files = [_pillow(frames[0], 60, 2, optimize=True), _pillow(frames[1], 90, 2, optimize=True), _pillow(frames[2], 75, 2)]
    assert ref.dht_tables(files[0]) != ref.dht_tables(files[1]) and ref.dqt_payloads(files[0]) != ref.dqt_payloads(files[1])
    together = ingest.decode_jpeg(files, DEV).cpu().numpy()
    for i in range(3):
        assert np.array_equal(together[i], _pillow_pixels(files[i])), i
        assert np.array_equal(ingest.decode_jpeg([files[i]], DEV).cpu().numpy()[0], together[i]), i
    perm = [2, 0, 1]
    assert np.array_equal(ingest.decode_jpeg([files[i] for i in perm], DEV).cpu().numpy(), together[perm])
    own = export.encode_jpeg(_dev(np.stack(frames)), quality=85, subsampling="4:4:4", huffman="optimized")
    assert np.array_equal(ingest.decode_jpeg(own, DEV).cpu().numpy(), np.stack([_pillow_pixels(d) for d in own]))


def test_a_noise_frame_whose_scan_spans_several_sequences():
    frame = ref.noise_frame(128, 192, 2)
    for sub in (0, 2):
        data = _pillow(frame, 100, sub)
        plain_bits = 8 * len(dec.unstuff(dec.parse(data)["scan"])[0])
        if sub == 0:
            assert plain_bits > 2 * _lib.load().tt_jpeg_sequence_bits(), plain_bits        # three sequences or more: the state is carried twice
        else:
            assert plain_bits > _lib.load().tt_jpeg_sequence_bits(), plain_bits
        raw, status = _decode_raw([data])
        assert status.tolist() == [0] and np.array_equal(raw[0], _pillow_pixels(data)), sub


def test_a_stuffed_pair_that_straddles_an_unstuffing_chunk():
    data = _pillow(ref.noise_frame(64, 96, 36), 100, 0)
    scan = dec.parse(data)["scan"]
    at = _lib.TT_JPEG_CHUNK * 5
    assert len(scan) > at and scan[at - 1] == 0xff and scan[at] == 0x00                   # the pair lies across chunks 4 and 5
    raw, status = _decode_raw([data, data])
    assert status.tolist() == [0, 0] and np.array_equal(raw[0], _pillow_pixels(data)) and np.array_equal(raw[1], raw[0])


def test_a_scan_cut_short_is_reported_and_its_neighbour_decodes():
    """A check of the length guards: the first frame's scan ends early at a byte boundary, with the true lengths passed."""
    files = [_pillow(ref.noise_frame(37, 53, 5), 90, 2), _pillow(ref.smooth_frame(37, 53, 6), 90, 2)]
    heads = [dec.parse(d) for d in files]
    cut = len(heads[0]["scan"]) // 2
    while heads[0]["scan"][cut - 1] == 0xff:                                           # not between an FF and its 00
        cut -= 1
    short = heads[0]["scan"][:cut]
    args = (dec.decode_set(heads[0]), heads[0]["dc"], heads[0]["ac"], 37, 53, 3, ref.S420)
    assert dec.entropy_lanes(short, *args)[1] != 0 and dec.entropy_sequential(short, *args)[1] != 0      # the emulation on the same input first
    sets = np.stack([ingest.jpeg_decode_set([hd["tables"][k] for k in (0x00, 0x10, 0x01, 0x11)], hd["dc"], hd["ac"]) for hd in heads])
    coeffs, status = _entropy_raw([short, heads[1]["scan"]], (37, 53, 3), ref.S420, sets)
    assert status[0] != 0 and status[0] == dec.entropy_lanes(short, *args)[1] and status[1] == 0
    pixels = _pixels_raw(coeffs, (37, 53, 3), ref.S420, np.stack([np.array(hd["quant"], dtype=np.uint8) for hd in heads]))
    assert np.array_equal(pixels[1], _pillow_pixels(files[1]))
    broken = files[0][:ingest.parse_jpeg(files[0]).scan_offset] + short + b"\xff\xd9"
    with pytest.raises(ValueError, match="frame 1 is corrupt or truncated"):
        ingest.decode_jpeg([files[1], broken], DEV)
    # an FF that no 00 follows, inside the scan: the parser never lets one through, the kernel reports it all the same
    marked = bytearray(heads[1]["scan"])
    marked[40:42] = b"\xff\x01"
    _, status = _entropy_raw([bytes(marked)], (37, 53, 3), ref.S420, sets[1:])
    assert status[0] & 1 and status[0] == dec.entropy_lanes(bytes(marked), *args)[1]


def test_ops_refuse_what_they_cannot_take():
    coeffs = torch.zeros((1, 12, 64), dtype=torch.int16, device=DEV)                  # 9 x 17 in 4:2:0: 2 MCUs of 6 blocks; 18 blocks in 4:4:4
    quant = torch.ones((1, 3, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="jpeg_pixels: coeffs must be"):
        ops.jpeg_pixels(coeffs, (9, 17, 3), "4:4:4", quant)
    with pytest.raises(RuntimeError, match="jpeg_pixels: quant must be"):
        ops.jpeg_pixels(coeffs, (9, 17, 3), "4:2:0", quant[0])
    scans = torch.zeros(64, dtype=torch.uint8, device=DEV)
    off, ln = torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((1,), 64, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="jpeg_entropy: tables must be"):
        ops.jpeg_entropy(scans, off, ln, 64, (9, 17, 3), "4:2:0", torch.zeros((1, 1024), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="jpeg_entropy: offsets int64"):
        ops.jpeg_entropy(scans, off.int(), ln, 64, (9, 17, 3), "4:2:0", torch.zeros((1, 1028), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="one geometry and subsampling per call"):
        ingest.decode_jpeg([_pillow(ref.smooth_frame(8, 8), 75, 0), _pillow(ref.smooth_frame(8, 16), 75, 0)], DEV)
    with pytest.raises(ValueError, match="progressive"):
        ingest.decode_jpeg([_pillow(ref.smooth_frame(8, 8), 75, 0, progressive=True)], DEV)

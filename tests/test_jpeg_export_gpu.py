"""GPU: the kernels of the JPEG export against the restatement of tests/jpeg_reference.py -- every coefficient, count, byte and length
equal -- on the smallest shapes at which they can go wrong: one pixel, one block, dummy Y blocks on the right (8 x 24) and at the bottom
(24 x 8), odd sizes, grey, both subsamplings, the qualities 1, 50, 75, 95 and 100, and shapes that span several of the units the
kernels cut a frame into: 128 x 192 (1152 blocks in 4:4:4: five workgroups of 256 blocks in the per-block kernels, two passes of the
1024-wide offset scan, several 4096-byte stuffing chunks on noise) and 24 x 520 (three 256-pixel tiles of the coefficient kernel).
The files of export.encode_jpeg byte for byte against the restatement, decoded by Pillow to the pixels of Pillow's own file; frame
independence; host against device copies; poison behind every buffer; optimized tables; write_jpegs' names and write_mjpeg's chunks.

Nothing here is a tolerance: the format is integers from end to end, so equality is the bound.  (The restatement itself is held to
Pillow's encoder in tests/test_jpeg_export_cpu.py.)"""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_reference as ref
from this_and_that_vdm_amd import _lib, export, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUBS = {"4:4:4": ref.S444, "4:2:0": ref.S420}

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def _pillow(frame, quality, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, optimize=False)
    return buf.getvalue()


SHAPES = [(1, 1, 3), (8, 8, 3), (8, 24, 3), (24, 8, 3), (9, 17, 3), (17, 9, 3), (15, 33, 3), (37, 53, 3), (64, 96, 3), (9, 17, 1),
          (128, 192, 3),          # several workgroups of 256 blocks, two passes of the 1024-wide scan, several stuffing chunks
          (24, 520, 3), (24, 520, 1)]          # three 256-pixel tiles of the coefficient kernel
QUALITIES = [1, 50, 75, 95, 100]


@functools.lru_cache(maxsize=None)
def _frames(shape):
    h, w, ch = shape
    return np.stack([ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch)], 0)


@functools.lru_cache(maxsize=None)
def _want(shape, quality, sub):
    """per frame of _frames(shape): (coefficients, counts, scan bytes) by the restatement -- computed once, shared by the tests"""
    out = []
    for frame in _frames(shape):
        coefs, comps, _ = ref.coefficients(frame, quality, sub)
        out.append((coefs, ref.symbol_counts(coefs, comps), ref.scan_bytes(coefs, comps)))
    return out


def _standard_tables():
    return _dev(np.stack([t.codes for t in export.jpeg_standard_tables()]).view(np.int32)[None])


# every shape in both subsamplings at all five qualities; the two tile-count shapes at 75
def _cases():
    return [(shape, sub, q) for shape in SHAPES for sub in SUBS for q in (QUALITIES if shape[1] != 520 else [75])]


CASES = _cases()


@pytest.mark.parametrize("shape,sub,quality", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_coefficients_counts_scan_and_lengths_equal_the_restatement(shape, sub, quality):
    frames = _frames(shape)
    want = _want(shape, quality, SUBS[sub])
    coeffs, counts = ops.jpeg_coeffs(_dev(frames), quality, sub)
    got_c, got_n = coeffs.cpu().numpy(), counts.cpu().numpy().view(np.uint32).astype(np.int64)
    assert got_c.shape == (2, ref.blocks_per_frame(*shape, SUBS[sub]), 64)
    for i in range(2):
        assert np.array_equal(got_c[i], want[i][0]), (i, np.argwhere(got_c[i] != want[i][0])[:5])
        assert np.array_equal(got_n[i], want[i][1]), (i, np.argwhere(got_n[i] != want[i][1])[:5])
    out, lengths = ops.jpeg_scan(coeffs, shape, sub, _standard_tables())
    out, lengths = out.cpu().numpy(), lengths.cpu().numpy()
    for i in range(2):
        assert int(lengths[i]) == len(want[i][2]), i
        assert out[i, :lengths[i]].tobytes() == want[i][2], i
    again = ops.jpeg_scan(coeffs, shape, sub, _standard_tables())
    assert np.array_equal(again[0].cpu().numpy()[0, :lengths[0]], out[0, :lengths[0]]) and np.array_equal(again[1].cpu().numpy(), lengths)


@pytest.mark.parametrize("shape,sub,quality", [((37, 53, 3), "4:2:0", 75), ((37, 53, 3), "4:4:4", 95), ((8, 24, 3), "4:2:0", 50), ((9, 17, 1), "4:2:0", 75),
                                               ((128, 192, 3), "4:2:0", 75), ((1, 1, 3), "4:4:4", 100)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_encode_jpeg_equals_the_restatements_file_and_decodes_as_pillows_own(shape, sub, quality):
    frames = _frames(shape)
    got = export.encode_jpeg(_dev(frames), quality=quality, subsampling=sub)
    assert len(got) == 2
    for i in range(2):
        assert got[i] == ref.jpeg_file(frames[i], quality, SUBS[sub]), i
        theirs = _pillow(frames[i], quality, SUBS[sub])
        assert np.array_equal(_decode(got[i]), _decode(theirs)), i
        assert ref.segments_of(got[i])[1] == ref.segments_of(theirs)[1] and ref.dqt_payloads(got[i]) == ref.dqt_payloads(theirs)
        if shape[2] == 3:
            assert got[i] == theirs                         # with the standard tables the whole file is Pillow's


def test_the_defaults_are_pillows_plain_save():
    from PIL import Image
    frame = ref.smooth_frame(37, 53, 4)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG")
    assert export.encode_jpeg(_dev(frame[None])) == [buf.getvalue()]


def test_frames_of_one_call_are_independent():
    frames = np.stack([ref.smooth_frame(37, 53, 1), ref.noise_frame(37, 53, 2), ref.checker_frame(37, 53)], 0)
    perm = [2, 0, 1]
    for huffman in ("standard", "optimized"):
        together = export.encode_jpeg(_dev(frames), huffman=huffman)
        assert export.encode_jpeg(_dev(frames[perm]), huffman=huffman) == [together[i] for i in perm]
        for i in range(3):
            assert export.encode_jpeg(_dev(frames[i:i + 1]), huffman=huffman) == [together[i]]


def test_host_and_device_copies_give_the_same_files():
    from PIL import Image
    frames = _frames((37, 53, 3))
    want = export.encode_jpeg(_dev(frames), quality=90, subsampling="4:4:4")
    assert export.encode_jpeg(frames, quality=90, subsampling="4:4:4") == want
    assert export.encode_jpeg([Image.fromarray(f) for f in frames], quality=90, subsampling="4:4:4") == want
    assert export.encode_jpeg(_dev(frames)[None], quality=90, subsampling="4:4:4") == want                  # a pipeline's output for one video
    assert export.encode_jpeg(torch.from_numpy(frames.astype(np.float32) / 255.0).to(DEV), quality=90, subsampling="4:4:4") == want
    grey = _frames((9, 17, 1))
    assert export.encode_jpeg(grey) == export.encode_jpeg(_dev(grey)) == [ref.jpeg_file(f, 75, ref.S420) for f in grey]


POISON = 0xA5


@pytest.mark.parametrize("shape,sub", [((37, 53, 3), "4:2:0"), ((128, 192, 3), "4:4:4"), ((9, 17, 1), "4:4:4")], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_poison_behind_every_buffer_stays(shape, sub):
    lib = _lib.load()
    frames = _frames(shape)
    n, (h, w, ch), s = 2, shape, SUBS[sub]
    blocks, stride, ws_bytes = lib.tt_jpeg_blocks(h, w, ch, s), lib.tt_jpeg_scan_bound(h, w, ch, s), lib.tt_jpeg_scan_ws_bytes(n, h, w, ch, s)
    tail = 4096

    def poisoned(nbytes):
        return torch.full((nbytes + tail,), POISON, dtype=torch.uint8, device=DEV)

    x = _dev(frames)
    coeffs, counts, out, lengths, ws = poisoned(n * blocks * 128), poisoned(n * 4096), poisoned(n * stride), poisoned(4 * n), poisoned(ws_bytes)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tt_jpeg_coeffs(x.data_ptr(), n, h, w, ch, 95, s, coeffs.data_ptr(), counts.data_ptr(), stream), "tt_jpeg_coeffs")
    _lib.check(lib.tt_jpeg_scan(coeffs.data_ptr(), n, h, w, ch, s, _standard_tables().data_ptr(), 1, out.data_ptr(), n * stride, lengths.data_ptr(),
                                ws.data_ptr(), ws_bytes, stream), "tt_jpeg_scan")
    torch.cuda.synchronize()
    for name, buf, used in (("coeffs", coeffs, n * blocks * 128), ("counts", counts, n * 4096), ("out", out, n * stride), ("lengths", lengths, 4 * n),
                            ("ws", ws, ws_bytes)):
        assert bool((buf[used:] == POISON).all()), name
    want = _want(shape, 95, s)
    got_len = lengths[:4 * n].cpu().numpy().view(np.int32)
    host = out.cpu().numpy()
    for i in range(n):
        assert int(got_len[i]) == len(want[i][2])
        assert host[i * stride:i * stride + got_len[i]].tobytes() == want[i][2]
        assert (host[i * stride + got_len[i]:(i + 1) * stride] == POISON).all()          # nothing at or beyond the length is written


@pytest.mark.parametrize("shape,sub,quality", [((37, 53, 3), "4:2:0", 75), ((64, 96, 3), "4:4:4", 95), ((9, 17, 1), "4:2:0", 50), ((128, 192, 3), "4:2:0", 75)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_optimized_tables(shape, sub, quality):
    frames = _frames(shape)
    got = export.encode_jpeg(_dev(frames), quality=quality, subsampling=sub, huffman="optimized")
    plain = export.encode_jpeg(_dev(frames), quality=quality, subsampling=sub)

    def library_tables(counts):
        return [(t.bits, t.huffval) for t in (export.jpeg_optimized_table(counts[k]) for k in range(4))]

    for i in range(2):
        assert got[i] == ref.jpeg_file(frames[i], quality, SUBS[sub], library_tables), i
        assert np.array_equal(_decode(got[i]), _decode(plain[i])), i
        assert len(got[i]) <= len(plain[i]), i


def test_write_jpegs_names_the_files_as_the_data_loaders_read_them(tmp_path):
    frames = np.stack([ref.smooth_frame(24, 40, s) for s in range(3)], 0)
    paths = export.write_jpegs(_dev(frames), str(tmp_path / "clip"))
    assert [os.path.basename(p) for p in paths] == ["im_0.jpg", "im_1.jpg", "im_2.jpg"]
    want = export.encode_jpeg(frames)
    for p, data in zip(paths, want):
        with open(p, "rb") as fh:
            assert fh.read() == data
    paths = export.write_jpegs(frames[:2], str(tmp_path / "clip"), pattern="{idx}.jpg", quality=90, subsampling="4:4:4")
    assert [os.path.basename(p) for p in paths] == ["0.jpg", "1.jpg"]
    with open(paths[1], "rb") as fh:
        assert fh.read() == ref.jpeg_file(frames[1], 90, ref.S444)
    with pytest.raises(ValueError, match="names two frames alike"):
        export.write_jpegs(frames, str(tmp_path / "clip"), pattern="same.jpg")


def test_write_mjpegs_chunks_are_encode_jpegs_bytes(tmp_path):
    frames = np.stack([ref.smooth_frame(24, 40, s) for s in range(3)], 0)
    path = str(tmp_path / "clip.avi")
    export.write_mjpeg(_dev(frames), path, fps=4, quality=80)
    want = export.encode_jpeg(frames, quality=80)
    assert export.read_mjpeg_frames(path) == want
    info = export.read_mjpeg(path)
    assert info["fps"] == 4 and info["total_frames"] == 3 and (info["width"], info["height"]) == (40, 24)
    buf = io.BytesIO()
    export.write_mjpeg(frames, buf, fps=4, quality=80)
    with open(path, "rb") as fh:
        assert fh.read() == buf.getvalue()
    for d in info["frames"]:
        assert _decode(d).shape == (24, 40, 3)


def test_ops_refuse_what_they_cannot_take():
    frames = _dev(_frames((9, 17, 3)))
    for kw, fragment in ((dict(quality=0), "quality"), (dict(quality=7.5), "quality"), (dict(subsampling="4:2:2"), "subsampling")):
        with pytest.raises(RuntimeError, match="jpeg_coeffs: " + fragment):
            ops.jpeg_coeffs(frames, **kw)
    with pytest.raises(RuntimeError, match="jpeg_coeffs: contiguous uint8"):
        ops.jpeg_coeffs(frames.float())
    with pytest.raises(RuntimeError, match="JPEG has no alpha"):
        ops.jpeg_coeffs(_dev(np.zeros((1, 8, 8, 4), dtype=np.uint8)))
    coeffs, _ = ops.jpeg_coeffs(frames, counts=False)
    with pytest.raises(RuntimeError, match="jpeg_scan: coeffs must be"):
        ops.jpeg_scan(coeffs, (9, 17, 3), "4:4:4", _standard_tables())
    with pytest.raises(RuntimeError, match="jpeg_scan: tables must be"):
        ops.jpeg_scan(coeffs, (9, 17, 3), "4:2:0", _standard_tables()[0])

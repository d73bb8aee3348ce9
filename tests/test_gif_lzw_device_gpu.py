"""GPU: tt_gif_lzw_frames against the host restatement of tests/gif_lzw_reference.py, byte for byte, on the smallest inputs at which the
kernels can go wrong: one and two pixels; segments of one pixel; a last segment shorter than the others; a segment count that is no
multiple of anything; per-frame min_code_size; a full table inside one segment (the cooperative clear, more than one staged chunk, more
than one pack tile); a closing code one bit wider than the code before it; data that ends on, before and behind a sub-block boundary.
Then what surrounds the bytes: batches, streams, poison around every buffer, the status words, the refusals with real buffers, and
export.write_gif(lzw="device") read back by Pillow.  Equality throughout; every case is tiny."""
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import gif_lzw_reference as lz
from tests import gif_lzw_refusals as refusals
from tests import gif_reference as ref
from this_and_that_vdm_amd import _lib, export, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


@functools.lru_cache(maxsize=None)
def _want_cached(raw, mcs, segment):
    return lz.restate(np.frombuffer(raw, dtype=np.uint8), mcs, segment)


def _want(frame, mcs, segment):
    """the restatement of one frame, computed once per (frame, min_code_size, segment)"""
    return _want_cached(np.ascontiguousarray(frame, dtype=np.uint8).tobytes(), int(mcs), segment)


def _run(frames, mcs, segment):
    """ops.gif_lzw on host frames -> (every frame's bytes, lengths, status)"""
    data, lengths, status = ops.gif_lzw(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), mcs, segment)
    data, lengths, status = data.cpu().numpy(), lengths.cpu().numpy(), status.cpu().numpy()
    return [data[i, :lengths[i]].tobytes() for i in range(len(lengths))], lengths, status


def _check(frames, mcs, segment):
    sizes = [mcs] * len(frames) if isinstance(mcs, int) else list(mcs)
    got, lengths, status = _run(frames, mcs, segment)
    assert not status.any(), status
    for i, frame in enumerate(frames):
        want = _want(frame, sizes[i], segment)
        assert lengths[i] == len(want) and got[i] == want, (i, segment, lengths[i], len(want))
    return got


SMALL = {"1 x 1": (1, 1), "1 x 2": (1, 2), "3 x 5": (3, 5)}


@pytest.mark.parametrize("segment", [1, 2, 7, None])
@pytest.mark.parametrize("name", list(SMALL))
@pytest.mark.parametrize("mcs", [2, 8])
def test_the_smallest_frames(name, segment, mcs):
    h, w = SMALL[name]
    _check(lz.random_indices(h * w, mcs, 40 + h * w).reshape(1, h, w), mcs, segment)


@pytest.mark.parametrize("segment", [64, 100, 384, 385, None])
def test_three_frames_with_a_min_code_size_each(segment):
    sizes = (2, 5, 8)
    frames = np.stack([lz.random_indices(384, m, 50 + m).reshape(16, 24) for m in sizes], 0)
    got = _check(frames, sizes, segment)
    for i, m in enumerate(sizes):                                             # a batch gives each frame the bytes it gets alone
        assert _run(frames[i:i + 1], m, segment)[0][0] == got[i]
    assert _run(frames, torch.tensor(sizes, dtype=torch.int32, device=DEV), segment)[0] == got      # the sizes as a device tensor


def test_a_full_table_inside_one_segment_equals_the_host_coder():
    frames = np.random.default_rng(7).integers(0, 256, size=(2, 96, 96)).astype(np.uint8)
    got = _check(frames, 8, 9216)
    for i in range(2):
        assert got[i] == export.lzw_frame(frames[i], 8)                       # rule 8
        assert ref.lzw_decode(got[i])[1] >= 3                                 # the first clear code and resets inside the segment
    _check(frames, 8, None)                                                   # the default: one segment as well
    _check(frames, 8, 8192)                                                   # ... and cut in two, with a shorter last segment
    _check(frames, 8, 4097)                                                   # a staged chunk and one pixel
    _check(lz.random_indices(20000, 8, 5)[None], 8, None)                     # more pixels than the built default: two segments


def test_a_constant_frame():
    frame = np.full((1, 64, 128), 3, dtype=np.uint8)
    got = _check(frame, 2, None)
    assert got[0] == export.lzw_frame(frame[0], 2)                            # one segment: the host coder's bytes
    _check(frame, 2, 1000)


def test_a_closing_code_one_bit_wider():
    px = lz.find_width_bump(2)
    two = np.concatenate([px, px])[None]
    _check(px[None], 2, None)                                                 # the end-of-information code is the wider one
    _check(two, 2, px.size)                                                   # a clear code between two segments is


@pytest.mark.parametrize("target", [254, 255, 256, 510])
def test_data_that_ends_around_a_sub_block_boundary(target):
    px = lz.find_data_bytes(target)
    got = _check(px[None], 8, 64)
    assert lz.data_bytes(got[0]) == target


def test_a_second_call_and_another_stream_give_the_same_bytes():
    frames = np.stack([lz.random_indices(384, 8, 60 + i).reshape(16, 24) for i in range(3)], 0)
    first = _check(frames, 8, 100)
    assert _run(frames, 8, 100)[0] == first
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _run(frames, 8, 100)[0]
    side.synchronize()
    assert other == first


# ---- what surrounds the bytes: the C entry point on buffers of the test's own
def _buffers(n, npix, segment, slack=256):
    lib = _lib.load()
    bound, ws_bytes = lib.tt_gif_lzw_frames_bound(npix, segment), lib.tt_gif_lzw_frames_ws_bytes(n, npix, segment)
    out = torch.full((slack + n * bound + slack,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((slack + ws_bytes + slack,), 0x5A, dtype=torch.uint8, device=DEV)
    small = torch.full((3, slack // 4 + n + slack // 4), 0x7B7B7B7B, dtype=torch.int32, device=DEV)      # mcs, lengths, status with their margins
    return lib, bound, ws_bytes, out, ws, small


def test_poison_around_every_buffer_stays():
    n, npix, segment, slack = 3, 384, 100, 256
    lib, bound, ws_bytes, out, ws, small = _buffers(n, npix, segment, slack)
    frames = np.stack([lz.random_indices(npix, 8, 70 + i) for i in range(n)], 0)
    idx = torch.from_numpy(frames).to(DEV)
    q = slack // 4
    small[0, q:q + n] = 8
    torch.cuda.synchronize()
    rc = lib.tt_gif_lzw_frames(idx.data_ptr(), n, npix, small[0, q:].data_ptr(), n, segment, out[slack:].data_ptr(), n * bound, small[1, q:].data_ptr(),
                               small[2, q:].data_ptr(), ws[slack:].data_ptr(), ws_bytes, None)
    assert rc == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    o, w, s = out.cpu().numpy(), ws.cpu().numpy(), small.cpu().numpy()
    assert (o[:slack] == 0xA5).all() and (o[slack + n * bound:] == 0xA5).all()
    assert (w[:slack] == 0x5A).all() and (w[slack + ws_bytes:] == 0x5A).all()
    assert (s[:, :q] == 0x7B7B7B7B).all() and (s[:, q + n:] == 0x7B7B7B7B).all() and (s[0, q:q + n] == 8).all()
    assert not s[2, q:q + n].any()
    for i in range(n):
        want = _want(frames[i], 8, segment)
        frame = o[slack + i * bound:slack + (i + 1) * bound]
        assert s[1, q + i] == len(want) and frame[:len(want)].tobytes() == want
        assert (frame[len(want):] == 0xA5).all()                             # nothing behind a frame's length, up to its stride


def test_an_index_out_of_range_marks_its_frame_alone():
    sizes = (5, 5, 5)
    frames = np.stack([lz.random_indices(384, 5, 80 + i).reshape(16, 24) for i in range(3)], 0)
    frames[1, 7, 3] = 32                                                      # does not fit min_code_size 5
    got, lengths, status = _run(frames, sizes, 100)
    assert status.tolist() == [0, _lib_status("INDEX"), 0]
    for i in (0, 2):
        assert got[i] == _want(frames[i], 5, 100)
    assert 0 < lengths[1] <= _lib.load().tt_gif_lzw_frames_bound(384, 100)
    with pytest.raises(ValueError, match="frame 1 "):
        export.lzw_frames_device(frames, sizes, 100)
    _, _, status = _run(frames, (5, 9, 1), 100)                               # min_code_size outside 2 .. 8: clamped and flagged
    assert status.tolist() == [0, _lib_status("MCS"), _lib_status("MCS") | _lib_status("INDEX")]      # clamped to 2, frame 2's indices do not fit
    assert export.lzw_frames_device(frames[::2], 5, 100) == [got[0], got[2]]  # host indices, one size for all


def _lib_status(name):
    return {"INDEX": 1, "MCS": 2}[name]


def test_every_refusal_with_real_buffers_leaves_them_alone():
    a0 = refusals.ARGS
    n_max = 4
    lib, bound, ws_bytes, out, ws, small = _buffers(n_max, a0["npix"], a0["segment"], 256)
    idx = torch.zeros((n_max, a0["npix"]), dtype=torch.uint8, device=DEV)
    small[0] = 8
    real = {"indices": idx.data_ptr(), "mcs": small[0, 64:].data_ptr(), "out": out[256:].data_ptr(), "lengths": small[1, 64:].data_ptr(),
            "status": small[2, 64:].data_ptr(), "ws": ws[256:].data_ptr()}
    fake = {k: a0[k] for k in real}
    torch.cuda.synchronize()
    for fault, code, fragment in refusals.ROWS:
        a = refusals.resolve(lib, dict(a0, **fault))
        for k in real:                                                        # the row's pointer, with its misalignment, onto a real buffer
            a[k] = None if a[k] is None else real[k] + (a[k] - fake[k])
        rc, msg = refusals.call(lib, a, None)
        assert rc == code and fragment in msg, (fault, rc, msg)
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (ws == 0x5A).all() and (small[1:] == 0x7B7B7B7B).all()


# ---- the exporter
def _decode(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    return im, np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)], 0)


def test_write_gif_on_the_device_route():
    frames = np.stack([ref.field_frame(32, 48, f, 6.0, np.random.default_rng(90 + f)) for f in range(14)], 0)
    dev = torch.from_numpy(frames).to(DEV)
    files = {}
    for name, src, kw in (("device", dev, dict(lzw="device")), ("device, host frames", frames, dict(lzw="device")), ("device again", dev, dict(lzw="device")),
                          ("device, 500", dev, dict(lzw="device", segment=500)), ("host", dev, dict(lzw="host")), ("default", dev, {})):
        buf = io.BytesIO()
        q = export.write_gif(src, buf, duration=0.05, **kw)
        files[name] = (buf.getvalue(), q)
    data, q = files["device"]
    im, decoded = _decode(data)
    assert im.n_frames == 14 and im.size == (48, 32) and np.array_equal(decoded, q.frames())
    assert np.array_equal(decoded, _decode(files["host"][0])[1])              # the same pixels as the host route's file
    assert files["device, host frames"][0] == data and files["device again"][0] == data
    assert files["host"][0] == files["default"][0]
    _, cut = _decode(files["device, 500"][0])
    assert np.array_equal(cut, decoded) and files["device, 500"][0] != data   # four segments a frame: other bytes, the same pixels
    for name in files:
        other = files[name][1]
        assert np.array_equal(other.indices, q.indices) and np.array_equal(other.palettes, q.palettes) and np.array_equal(other.frame_sse, q.frame_sse)
    # 1536 pixels a frame are one segment at the default: the device route's file is the host route's
    assert data == files["host"][0]
    again = io.BytesIO()
    export.write_gif_indexed(q.indices, q.palettes, q.ncolors, again, duration=0.05, palette=q.palette, lzw="device", segment=500)
    assert again.getvalue() == files["device, 500"][0]
    with pytest.raises(ValueError, match="lzw"):
        export.write_gif(dev, io.BytesIO(), lzw="gpu")

"""GPU: the PNG import of include/ttvdm.h ("PNG import"), byte for byte against the restatement of tests/png_decode_reference.py and,
where Pillow can read the file, against Pillow: the inflate on arbitrary bytes (zlib's outputs at every strategy) and on hand-built
streams, each with the property it is there for read back from its tokens; the unfilter as the inverse of ``ops.png_filter``; whole
files; every status bit on a stream built for it; poisoned bytes around the buffers; a corrupt neighbour; two calls and a side stream;
the refusals with real buffers.  No tolerance anywhere."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch

from tests import png_decode_reference as g
from this_and_that_vdm_amd.ingest import decode_png, read_apng, read_pngs          # the feature under test: without it nothing here is collected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def inflate(streams, expected, slack=0):
    """-> (per stream its bytes, the status words, the whole out buffer) of one tt_png_inflate call; stream f's bytes go to a multiple of
    16 behind stream f - 1's, ``slack`` bytes in front of the first"""
    from this_and_that_vdm_amd import ops
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    exp = np.array(expected, dtype=np.int64)
    stride = (exp + 15) // 16 * 16
    oo = slack + np.concatenate([[0], np.cumsum(stride)[:-1]])
    out, status = ops.png_inflate(dev(np.frombuffer(b"".join(streams), dtype=np.uint8), np.uint8), dev(offs, np.int64), dev(lens, np.int32), dev(exp, np.int32),
                                  dev(oo, np.int64), int(exp.max()), int(slack + stride.sum() + slack))
    host = out.cpu().numpy()
    return [host[o:o + e].tobytes() for o, e in zip(oo, exp)], status.cpu().tolist(), out


@functools.lru_cache(maxsize=None)
def reference(kind):
    """the restatement's answers, computed once: name -> (stream, out, status, blocks)"""
    cases = {"encoder": g.encoder_cases, "handbuilt": g.handbuilt_cases}[kind]()
    return {name: (stream, prop, g.inflate(stream)) for name, stream, prop in cases}


ENCODER = [c[0] for c in g.encoder_cases()]
HANDBUILT = [c[0] for c in g.handbuilt_cases()]


@pytest.mark.parametrize("name", ENCODER)
def test_inflate_of_zlibs_output_on_arbitrary_bytes(name):
    stream, prop, want = reference("encoder")[name]
    assert prop(want["blocks"]), "the encoder no longer gives this stream the property the case relies on"
    got, status, _ = inflate([stream], [len(want["out"])])
    assert status == [0] and got[0] == want["out"] == zlib.decompress(stream)


@pytest.mark.parametrize("name", HANDBUILT)
def test_inflate_of_a_hand_built_stream(name):
    stream, prop, want = reference("handbuilt")[name]
    assert prop(want["blocks"]) and want["status"] == 0
    got, status, _ = inflate([stream], [len(want["out"])])
    assert status == [0] and got[0] == want["out"] == zlib.decompress(stream)


def test_a_constant_stream_is_one_chain_as_long_as_the_stream():
    n = 70001
    stream = zlib.compress(bytes([7]) * n, 9)
    tokens = g.all_tokens(g.inflate(stream)["blocks"])
    copies = [t for t in tokens if isinstance(t, tuple)]
    assert tokens[0] == 7 and {t[1] for t in copies} == {1} and sum(t[0] for t in copies) >= n - 4      # all but a few bytes name the one before them
    got, status, _ = inflate([stream], [n])
    assert status == [0] and got[0] == bytes([7]) * n


@pytest.mark.parametrize("case", g.corrupt_cases(), ids=[c[0] for c in g.corrupt_cases()])
def test_every_status_bit_is_raised_by_the_stream_built_for_it(case):
    name, stream, expected, want = case
    ref = g.inflate(stream, expected)
    assert ref["status"] == want
    got, status, _ = inflate([stream], [expected])
    assert status == [want] and got[0] == ref["out"]


def test_a_span_outside_the_uploaded_bytes_marks_only_its_own_stream():
    from this_and_that_vdm_amd import ops
    a, b = zlib.compress(g.text(3000, 1)), zlib.compress(g.noise(2000, 2))
    data = dev(np.frombuffer(a + b, dtype=np.uint8), np.uint8)
    for fault in (dict(offsets=[0, len(a) + 1]), dict(lengths=[len(a), len(b) + 1]), dict(offsets=[0, -1]), dict(expected=[3000, 3009]), dict(out_offsets=[0, 5000])):
        args = dict(offsets=[0, len(a)], lengths=[len(a), len(b)], expected=[3000, 2000], out_offsets=[0, 3008])
        args.update(fault)
        out, status = ops.png_inflate(data, dev(args["offsets"], np.int64), dev(args["lengths"], np.int32), dev(args["expected"], np.int32), dev(args["out_offsets"], np.int64),
                                      3008, 3008 + 2000)
        assert status.cpu().tolist() == [0, g.SPAN], fault
        assert out[:3000].cpu().numpy().tobytes() == g.text(3000, 1), fault


def test_a_corrupt_neighbour_leaves_the_other_streams_bit_equal_and_poison_around_the_buffers_stays():
    from this_and_that_vdm_amd import _lib, ops
    good = [zlib.compress(g.text(5000, 3), 9), zlib.compress(g.noise(4000, 4), 0), g.handbuilt_cases()[0][1], zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)]
    good[3] = good[3].compress(g.text(900, 5)) + good[3].flush()
    sizes = [len(zlib.decompress(s)) for s in good]
    clean, status, _ = inflate(good, sizes)
    assert status == [0] * 4 and [zlib.decompress(s) for s in good] == clean
    for name, stream, expected, want in g.corrupt_cases()[::3]:
        mixed = good[:2] + [stream] + good[2:]
        got, status, _ = inflate(mixed, sizes[:2] + [expected] + sizes[2:])
        assert status == [0, 0, want, 0, 0] and got[:2] + got[3:] == clean, name
    # poison: the call through the C ABI on buffers with guard bytes before and behind data, out, status and the workspace
    lib = _lib.load()
    n, guard = len(good), 256
    lens, exp = np.array([len(s) for s in good]), np.array(sizes)
    stride = (exp + 15) // 16 * 16
    out_bytes = int(stride.sum())
    ws_bytes = lib.tt_png_decode_ws_bytes(n, out_bytes, int(exp.max()))
    bufs = {k: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device=DEV) for k, size in (("out", out_bytes), ("status", 4 * n), ("ws", ws_bytes))}
    data = dev(np.frombuffer(b"".join(good), dtype=np.uint8), np.uint8)
    offs, oo = dev(np.concatenate([[0], np.cumsum(lens)[:-1]]), np.int64), dev(np.concatenate([[0], np.cumsum(stride)[:-1]]), np.int64)
    lens_d, exp_d = dev(lens, np.int32), dev(exp, np.int32)           # held: a temporary's memory is the next temporary's
    rc = lib.tt_png_inflate(data.data_ptr(), data.numel(), offs.data_ptr(), lens_d.data_ptr(), exp_d.data_ptr(), oo.data_ptr(), n, int(exp.max()),
                            bufs["out"].data_ptr() + guard, out_bytes, bufs["status"].data_ptr() + guard, bufs["ws"].data_ptr() + guard, ws_bytes,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.tt_last_error()
    for k, b in bufs.items():
        assert bool((b[:guard] == 0xA5).all()) and bool((b[-guard:] == 0xA5).all()), k + ": a guard byte changed"
    host = bufs["out"][guard:-guard].cpu().numpy()
    at = 0
    for f in range(n):
        assert host[at:at + sizes[f]].tobytes() == clean[f]
        assert (host[at + sizes[f]:at + int(stride[f])] == 0xA5).all()                              # the padding between two streams is not written
        at += int(stride[f])
    assert bufs["status"][guard:-guard].view(torch.int32).cpu().tolist() == [0] * n


def test_two_calls_and_a_call_on_a_side_stream_give_the_same_bytes():
    streams = [c[1] for c in g.encoder_cases()[3:7]]
    sizes = [len(zlib.decompress(s)) for s in streams]
    first, status, _ = inflate(streams, sizes)
    second, _, _ = inflate(streams, sizes)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third, status3, _ = inflate(streams, sizes)
    side.synchronize()
    assert status == status3 == [0] * 4 and first == second == third == [zlib.decompress(s) for s in streams]


# ---- the unfilter
def tie_rows(ch):
    """rows built for Paeth's three-way ties (a = b = c, and a + b - c at equal distances) and Average sums above 255"""
    rows = np.zeros((6, 12, ch), dtype=np.uint8)
    rows[0] = 200
    rows[1] = 200                                                     # a = b = c: every distance is 0
    rows[2, ::2], rows[2, 1::2] = 10, 250                             # left and up far apart
    rows[3, ::2], rows[3, 1::2] = 250, 10
    rows[4] = (np.arange(12)[:, None] * 7 + 130) % 256                     # a + b above 255 on most pixels
    rows[5] = 255
    return rows


BAND = 256
SHAPES = [(1, 1), (1, 7), (7, 1), (13, 17), (BAND + 1, 3), (2 * BAND + 5, 2), (3, BAND + 1)]


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_unfilter_is_the_inverse_of_filter_for_every_type(ch):
    from this_and_that_vdm_amd import _lib, ops
    assert _lib.TT_PNG_UNFILTER_BAND == BAND
    for h, w in SHAPES:
        frames = np.stack([g.picture(h, w, ch, 1, smooth=False), g.picture(h, w, ch, 2, smooth=True)])
        x = dev(frames, np.uint8)
        for k in range(6):
            filtered = ops.png_filter(x, filter=k)
            y, status = ops.png_unfilter(filtered, (h, w, ch))
            assert status.cpu().tolist() == [0, 0] and torch.equal(x, y), (h, w, k)
    x = dev(tie_rows(ch)[None], np.uint8)
    for k in (3, 4, 5):
        filtered = ops.png_filter(x, filter=k)
        y, _ = ops.png_unfilter(filtered, (6, 12, ch))
        stream = filtered[0].cpu().numpy().tobytes()
        assert torch.equal(x, y) and np.array_equal(g.unfilter(stream, 6, 12, ch)[0], tie_rows(ch)), k


def test_unfilter_of_mixed_rows_equals_the_restatement_and_names_a_bad_type():
    from this_and_that_vdm_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(3)
    h, w, ch = 2 * BAND + 9, 5, 3
    px = g.picture(h, w, ch, 4, smooth=False)
    kinds = [int(k) for k in rng.integers(0, 5, size=h)]
    kinds[BAND], kinds[2 * BAND] = 4, 1                               # one band that leans on the band before it, one that starts on its own
    stream = bytearray(g.filter_rows(px, kinds))
    stride = lib.tt_png_frame_stride(h, w, ch)
    spoiled = bytearray(stream)
    spoiled[7 * (1 + w * ch)] = 5                                     # row 7's type byte
    both = np.zeros((2, stride), dtype=np.uint8)
    both[0, :len(stream)], both[1, :len(stream)] = np.frombuffer(bytes(stream), dtype=np.uint8), np.frombuffer(bytes(spoiled), dtype=np.uint8)
    y, status = ops.png_unfilter(dev(both, np.uint8), (h, w, ch))
    want, bad = g.unfilter(bytes(spoiled), h, w, ch)
    assert bad == 1 and status.cpu().tolist() == [0, 1]
    assert np.array_equal(y[0].cpu().numpy(), px) and np.array_equal(y[1].cpu().numpy(), want)


# ---- whole files
@pytest.mark.parametrize("name", [c[0] for c in g.file_cases()])
def test_a_file_equals_pillow_and_the_restatement(name):
    data = dict(g.file_cases())[name]
    got = decode_png(data, DEV)
    want = g.pillow_pixels(data)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (1, *want.shape)
    assert np.array_equal(got.cpu().numpy()[0], want) and np.array_equal(g.decode(data)[0], want)


@pytest.mark.parametrize("filter", ["none", "sub", "up", "average", "paeth", "adaptive"])
def test_files_of_encode_png_at_every_filter_setting(filter, tmp_path):
    from this_and_that_vdm_amd import export
    frames = np.stack([g.picture(37, 29, 3, s, smooth=s % 2 == 0) for s in range(3)])
    files = export.encode_png(dev(frames, np.uint8), filter=filter)
    got = decode_png(files, DEV).cpu().numpy()
    assert np.array_equal(got, frames) and all(np.array_equal(g.pillow_pixels(f), frames[i]) for i, f in enumerate(files))
    if filter == "adaptive":
        export.write_pngs(dev(frames, np.uint8), str(tmp_path))
        assert np.array_equal(read_pngs(str(tmp_path), device=DEV).cpu().numpy(), frames)
        with pytest.raises(ValueError, match="does not exist"):
            read_pngs(str(tmp_path / "nowhere"), device=DEV)


def test_write_apng_read_back_by_read_apng_and_its_default_image_by_decode_png(tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd import export
    frames = np.stack([g.picture(21, 34, 3, s) for s in range(4)])
    path = str(tmp_path / "clip.png")
    export.write_apng(dev(frames, np.uint8), path)
    assert np.array_equal(read_apng(path, DEV).cpu().numpy(), frames)
    assert np.array_equal(decode_png(path, DEV).cpu().numpy()[0], np.asarray(Image.open(path)))      # the default image, as Image.open shows it
    with Image.open(path) as im:
        assert im.n_frames == 4
        for f in range(4):
            im.seek(f)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[f])


def test_a_batch_mixing_stream_kinds_in_one_call_and_a_corrupt_file_named():
    px = [g.picture(33, 47, 3, s, smooth=s != 1) for s in range(5)]          # Z_FIXED gives noise stored blocks: file 2 is smooth
    rb = 1 + 47 * 3
    raw = [g.filter_rows(p, [s % 5] * 33) for s, p in enumerate(px)]
    files = [g.pillow_png(px[0]), g.pillow_png(px[1], compress_level=0), g.png_file(47, 33, 2, g.compress(raw[2], 6, strategy=zlib.Z_FIXED)),
             g.rechunk(g.png_file(47, 33, 2, g.compress(raw[3], 9, wbits=9)), size=7), g.png_file(47, 33, 2, g.compress(raw[4], 1, flush_every=rb))]
    kinds = [g.kinds_of(g.inflate(g.parse(f)["idat"])["blocks"]) for f in files]
    assert kinds[1] == {"stored"} and kinds[2] == {"fixed"} and "dynamic" in kinds[0] and len(g.parse(files[3])["spans"]) > 20
    got = decode_png(files, DEV).cpu().numpy()
    assert np.array_equal(got, np.stack(px))
    hd = g.parse(files[2])
    broken = bytearray(hd["idat"])
    broken[-1] ^= 0x40
    from PIL import Image
    with pytest.raises(OSError):
        Image.open(io.BytesIO(g.png_file(47, 33, 2, bytes(broken)))).load()
    with pytest.raises(ValueError, match=r"decode_png: file 2 is corrupt or truncated \(an Adler-32 mismatch; status 32, rows 0\)"):
        decode_png(files[:2] + [g.png_file(47, 33, 2, bytes(broken))] + files[3:], DEV)
    with pytest.raises(ValueError, match=r"file 0 is corrupt or truncated \(fewer bytes than the image holds"):
        decode_png(g.png_file(47, 34, 2, hd["idat"]), DEV)


def test_the_refusals_with_real_buffers():
    from this_and_that_vdm_amd import _lib, ops
    lib = _lib.load()
    stream = zlib.compress(g.text(1000, 1))
    data, one64, one32 = dev(np.frombuffer(stream, dtype=np.uint8), np.uint8), dev([0], np.int64), dev([len(stream)], np.int32)
    with pytest.raises(RuntimeError, match="max_out = 2000 above out_bytes = 1008"):
        ops.png_inflate(data, one64, one32, dev([1000], np.int32), one64, 2000, 1008)
    with pytest.raises(RuntimeError, match="expected must be a contiguous torch.int32"):
        ops.png_inflate(data, one64, one32, dev([1000], np.int64), one64, 1000, 1008)
    with pytest.raises(RuntimeError, match="max_out 0"):
        ops.png_inflate(data, one64, one32, dev([1000], np.int32), one64, 0, 1008)
    out, status, ws = torch.empty(1008, dtype=torch.uint8, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(64, dtype=torch.uint8, device=DEV)
    exp_d = dev([1000], np.int32)
    rc = lib.tt_png_inflate(data.data_ptr(), data.numel(), one64.data_ptr(), one32.data_ptr(), exp_d.data_ptr(), one64.data_ptr(), 1, 1000, out.data_ptr(),
                            1008, status.data_ptr(), ws.data_ptr(), 64, None)
    assert rc != 0 and b"ws too small: 64 bytes" in lib.tt_last_error()
    with pytest.raises(RuntimeError, match=r"png_unfilter: filtered must be a contiguous uint8 tensor \[N, 64\]"):
        ops.png_unfilter(torch.zeros((1, 63), dtype=torch.uint8, device=DEV), (4, 5, 3))
    with pytest.raises(RuntimeError, match="1 to 4 channels"):
        ops.png_unfilter(torch.zeros((1, 64), dtype=torch.uint8, device=DEV), (4, 5, 5))

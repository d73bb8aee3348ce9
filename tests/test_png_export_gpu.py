"""GPU: the three kernels of the PNG export against the restatement of tests/png_reference.py -- every byte equal -- on the smallest
shapes at which they can go wrong: every filter type and the adaptive choice on one pixel, one row, one column, odd sizes and 1, 3 and
4 channels; run lengths around every threshold of the token rule (3, 258, 259 .. 262, 517, a whole stripe), a run across a stripe
boundary, streams of exactly one and two stripes and two stripes and a byte, a stripe of 255s for the Adler sums; the files of
export.encode_png byte for byte against the restatement fed the library's code lengths, decoded by Pillow to the exact pixels;
write_pngs' names and write_apng's frames.

Nothing here is a tolerance: the format is lossless and every rule is closed, so equality is the bound.  (The files' sizes against
Pillow's are held on the restatement, tests/test_png_export_cpu.py.)"""
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import png_reference as ref
from this_and_that_vdm_amd import _lib, export, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


def _rand(shape, seed, high=256):
    return np.random.default_rng(seed).integers(0, high, size=shape, dtype=np.int64).astype(np.uint8)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _lib_lengths(counts, limit):
    return export.png_code_lengths(counts, limit)


# ---- the filter
def _filtered(frames, kind):
    n, h, w, ch = frames.shape
    out = ops.png_filter(_dev(frames), kind).cpu().numpy()
    size = h * (1 + w * ch)
    assert out.shape == (n, (size + 15) // 16 * 16)
    return out[:, :size]


FILTER_SHAPES = [(1, 1, 1, 3), (1, 1, 7, 3), (1, 5, 1, 3), (1, 9, 97, 3), (1, 64, 96, 3), (1, 9, 97, 1), (1, 9, 97, 4), (2, 9, 97, 2)]


@pytest.mark.parametrize("kind", range(6), ids=["none", "sub", "up", "average", "paeth", "adaptive"])
@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_png_filter_equals_the_restatement(shape, kind):
    n, h, w, ch = shape
    frames = np.stack([ref.generator_frame(h, w, 7 + i, ch) if h * w > 40 else _rand((h, w, ch), 7 + i) for i in range(n)], 0)
    got = _filtered(frames, kind)
    for i in range(n):
        want, _ = ref.filter_frame(frames[i], kind)
        assert np.array_equal(got[i], want), i


def test_frames_of_one_call_are_independent():
    frames = np.stack([ref.generator_frame(9, 97, s) for s in (1, 2, 3)], 0)
    perm = [2, 0, 1]
    a, b = _filtered(frames, 5), _filtered(frames[perm], 5)
    assert np.array_equal(a[perm], b)
    for i in range(3):
        assert np.array_equal(a[i], _filtered(frames[i:i + 1], 5)[0])
        assert np.array_equal(a[i], ref.filter_frame(frames[i], 5)[0])


def test_a_row_whose_costs_tie_takes_the_lowest_type():
    frames = np.zeros((1, 4, 6, 3), dtype=np.uint8)
    frames[0, 2] = 128                              # x - a = 128 for the first pixel, 0 then; up: 128 everywhere: |128| counts 128 either way
    got = _filtered(frames, 5)[0].reshape(4, 19)
    want, types = ref.filter_frame(frames[0], 5)
    assert np.array_equal(got.reshape(-1), want) and got[:, 0].tolist() == types and types[0] == 0 and types[1] == 0


def test_names_select_the_filter_and_others_are_refused():
    frames = _rand((1, 5, 6, 3), 3)
    assert np.array_equal(_filtered(frames, "paeth"), _filtered(frames, 4)) and np.array_equal(_filtered(frames, "adaptive"), _filtered(frames, 5))
    for bad in ("best", 6, -1, 2.0):
        with pytest.raises(RuntimeError, match="png_filter: filter"):
            ops.png_filter(_dev(frames), bad)
    with pytest.raises(RuntimeError, match="png_filter: contiguous uint8"):
        ops.png_filter(_dev(frames).float(), 5)


# ---- tokens: with filter 0, one channel and one row the stream is a 0 followed by the row, so the test dictates the bytes
def _runs(lengths, seed):
    """a stream that starts with the filter byte 0 and goes on with runs of the given lengths; neighbouring runs differ"""
    rng = np.random.default_rng(seed)
    out, last = [np.zeros(1, dtype=np.uint8)], 0
    for n in lengths:
        v = int(rng.integers(1, 256))
        v = v if v != last else (v % 255) + 1
        out.append(np.full(n, v, dtype=np.uint8))
        last = v
    return np.concatenate(out)


def _noise_with_runs(n, seed):
    s = _rand(n, seed, high=4)                      # four values: plenty of short runs
    s[0] = 0
    return s


def _stream_cases():
    S = ref.STRIPE
    cross = _noise_with_runs(S + 700, 31)
    cross[S - 300:S + 300] = 9                     # one run over the stripe boundary: two runs of 300, one in each stripe
    edge = _noise_with_runs(2 * S, 32)
    edge[S - 1], edge[S] = 5, 5                    # equal bytes on both sides of the boundary, single on each
    ff = np.concatenate([_noise_with_runs(S, 33), np.full(S, 255, dtype=np.uint8)])
    # Fibonacci counts: the filter byte and the end of block are the 1, 1
    fib = np.concatenate([np.full(c, 3 + i, dtype=np.uint8) for i, c in enumerate([2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987,
                                                                                    1597, 2584, 4181, 6765, 10946])])
    spread = np.empty_like(fib)                     # the values in descending frequency over the even places, then the odd ones: no two
    spread[np.concatenate([np.arange(0, fib.size, 2), np.arange(1, fib.size, 2)])] = fib[::-1]      # neighbours are equal, every byte a literal
    fib = np.concatenate([np.zeros(1, dtype=np.uint8), spread])
    return {
        "runs of 1 2 3 4 258 259 260 261 262 517": _runs([1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 1, 1, 2, 5], 30),
        "a run of 32768: one stripe of zeros": np.zeros(S, dtype=np.uint8),
        "a run of 32767 behind the filter byte": np.concatenate([np.zeros(1, dtype=np.uint8), np.full(S - 1, 200, dtype=np.uint8)]),
        "a run across the stripe boundary": cross,
        "exactly one stripe": _noise_with_runs(S, 35),
        "exactly two stripes, equal bytes at the boundary": edge,
        "two stripes and one byte": _noise_with_runs(2 * S + 1, 36),
        "a stripe of 255s": ff,
        "one byte short of a stripe": _noise_with_runs(S - 1, 37),
        "a fibonacci stripe": fib,
        "uniform noise": np.concatenate([np.zeros(1, dtype=np.uint8), _rand(40000, 38)]),
        "three bytes": np.array([0, 4, 4], dtype=np.uint8),
    }


STREAMS = _stream_cases()


def _frame_of(stream):
    assert stream[0] == 0
    return stream[1:].reshape(1, 1, -1, 1)


@functools.lru_cache(maxsize=None)
def _want_records(name):
    return np.stack([ref.record_of(p) for p in ref.stripes_of(STREAMS[name])])


@functools.lru_cache(maxsize=None)
def _want_file(name):
    return ref.png_file(_frame_of(STREAMS[name])[0], 0, _lib_lengths)


@pytest.mark.parametrize("name", list(STREAMS))
def test_png_tokens_records_equal_the_restatement(name):
    stream = STREAMS[name]
    frames = _frame_of(stream)
    filtered = ops.png_filter(_dev(frames), 0)
    assert np.array_equal(filtered.cpu().numpy()[0, :stream.size], stream)
    shape = frames.shape[1:]
    got = ops.png_tokens(filtered, shape).cpu().numpy().view(np.uint32).astype(np.int64)
    want = _want_records(name)
    assert got.shape == want.shape
    assert np.array_equal(got[:, :286], want[:, :286]), np.argwhere(got[:, :286] != want[:, :286])[:5]
    assert np.array_equal(got[:, 286:], want[:, 286:])
    assert (got[:, 256] == 1).all()
    assert np.array_equal(ops.png_tokens(filtered, shape).cpu().numpy().view(np.uint32), got)      # the same bits on a second call


def test_the_fibonacci_stripe_reaches_the_length_limit():
    lengths = _lib_lengths(_want_records("a fibonacci stripe")[0, :286], 15)
    assert int(lengths.max()) == 15 and int(ref.package_merge(_want_records("a fibonacci stripe")[0, :286], 32).max()) > 15


def test_tokens_of_several_frames_in_one_launch():
    frames = np.stack([ref.generator_frame(150, 96, s) for s in (4, 5)], 0)         # 150 x 289 bytes: two stripes a frame, the second short
    filtered = ops.png_filter(_dev(frames), 5)
    got = ops.png_tokens(filtered, frames.shape[1:]).cpu().numpy().view(np.uint32).astype(np.int64)
    want = np.concatenate([np.stack([ref.record_of(p) for p in ref.stripes_of(ref.filter_frame(f, 5)[0])]) for f in frames])
    assert got.shape == (4, 288) and np.array_equal(got, want)


# ---- the files
def _check_file(data, frame):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    back = np.asarray(im)
    assert np.array_equal(back if back.ndim == 3 else back[..., None], frame)


@pytest.mark.parametrize("name", list(STREAMS))
def test_encode_png_equals_the_restatements_file(name):
    frames = _frame_of(STREAMS[name])
    got = export.encode_png(_dev(frames), filter="none")
    assert len(got) == 1 and got[0] == _want_file(name)
    _check_file(got[0], frames[0])
    assert export.encode_png(frames, filter=0) == got                       # a host copy of the frames, and a second call


GENERATED = np.stack([ref.generator_frame(64, 96, s) for s in (0, 1, 2)], 0)


@pytest.mark.parametrize("kind", ["adaptive", "paeth", "none"])
def test_encode_png_of_the_generators_frames(kind):
    got = export.encode_png(_dev(GENERATED), filter=kind)
    assert len(got) == 3
    for i in range(3):
        assert got[i] == ref.png_file(GENERATED[i], ops.PNG_FILTERS[kind], _lib_lengths), i
        _check_file(got[i], GENERATED[i])
    assert export.encode_png(GENERATED, filter=kind) == got and export.encode_png(_dev(GENERATED), filter=kind) == got
    from PIL import Image
    assert export.encode_png([Image.fromarray(f) for f in GENERATED], filter=kind) == got
    assert export.encode_png(_dev(GENERATED)[None], filter=kind) == got    # a pipeline's output for one video


@pytest.mark.parametrize("ch", [1, 2, 4])
def test_encode_png_of_other_channel_counts_and_float_frames(ch):
    frames = np.stack([ref.generator_frame(33, 47, s, ch) for s in (0, 1)], 0)
    got = export.encode_png(_dev(frames))
    for i in range(2):
        assert got[i] == ref.png_file(frames[i], 5, _lib_lengths)
        _check_file(got[i], frames[i])
    as_float = torch.from_numpy(frames.astype(np.float32) / 255.0).to(DEV)
    assert export.encode_png(as_float) == got                               # rounded back to the same bytes


def test_a_stream_of_several_chunks_of_bits():
    """uniform noise costs about 8 bits a byte: a full stripe is two 16 KiB chunks of the emit kernel's LDS staging, and stripes start
    at every offset inside a 16-byte unit of the output"""
    frames = _rand((3, 101, 131, 3), 41)
    got = export.encode_png(_dev(frames), filter="up")
    for i in range(3):
        assert got[i] == ref.png_file(frames[i], 2, _lib_lengths), i
        _check_file(got[i], frames[i])


def test_write_pngs_names_the_files_as_the_reference_does(tmp_path):
    paths = export.write_pngs(_dev(GENERATED), str(tmp_path / "out"))
    assert [os.path.basename(p) for p in paths] == ["0.png", "1.png", "2.png"]
    want = export.encode_png(GENERATED)
    for p, data in zip(paths, want):
        with open(p, "rb") as fh:
            assert fh.read() == data
    paths = export.write_pngs(GENERATED[:2], str(tmp_path / "out"), pattern="frame_{idx:03d}.png", filter="sub")
    assert [os.path.basename(p) for p in paths] == ["frame_000.png", "frame_001.png"]
    with pytest.raises(ValueError, match="names two frames alike"):
        export.write_pngs(GENERATED, str(tmp_path / "out"), pattern="same.png")


def test_write_apng_opens_in_pillow_with_every_frame_exact(tmp_path):
    from PIL import Image
    path = str(tmp_path / "combined.png")
    export.write_apng(_dev(GENERATED), path, duration=0.05, loop=0)
    im = Image.open(path)
    assert im.n_frames == 3 and im.size == (96, 64) and im.info.get("loop") == 0
    for i in range(3):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), GENERATED[i]), i
        assert im.info.get("duration") == 50.0
    with open(path, "rb") as fh:
        chunks = ref.chunks_of(fh.read())
    assert [c[0] for c in chunks] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"] and all(c[2] for c in chunks)
    single = export.encode_png(GENERATED)
    assert chunks[3][1] == ref.chunks_of(single[0])[1][1] and chunks[5][1][4:] == ref.chunks_of(single[1])[1][1]      # the same streams
    buf = io.BytesIO()
    export.write_apng(GENERATED[:1], buf, duration=0.1, loop=2)
    assert Image.open(io.BytesIO(buf.getvalue())).n_frames == 1

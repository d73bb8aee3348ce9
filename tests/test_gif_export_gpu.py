"""GPU: tt_color_hist and tt_palette_map against the numpy restatements of tests/gif_reference.py -- every integer equal -- on the
smallest shapes at which the kernels can go wrong (odd sizes, frames that start off a 16-byte boundary, a tail shorter than the 16
pixels of a lane's loads, more than one workgroup per frame, more distinct bins than the private table has slots, one bin for every
pixel); export.quantize_frames with Lloyd iterations against the restatement; the file write_gif writes, read back by Pillow; and the
quality condition against Pillow's own median cut.

The Lloyd bound sse_after <= sse_before + 0.75 pixels is derived, not measured: reassigning every pixel to its nearest entry cannot raise
the sum, moving an entry to the exact centroid of its pixels cannot raise it, and rounding the centroid by at most 1/2 per channel adds
at most 1/4 per pixel and channel (sum |x - (c + e)|^2 = sum |x - c|^2 + n e^2 about the centroid c)."""
import io
import os

import numpy as np
import pytest
import torch

from tests import gif_reference as ref
from this_and_that_vdm_amd import _lib, export, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.int64).astype(np.uint8)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _hist(frames, per_frame):
    return ops.color_hist(_dev(frames), per_frame=per_frame).cpu().numpy().view(np.uint32).astype(np.int64)


def _every_bin_once():
    bins = np.arange(ref.BINS)
    px = np.stack([((bins >> s) & 31) << 3 for s in (10, 5, 0)], 1) + np.random.default_rng(1).integers(0, 8, size=(ref.BINS, 3))
    return np.random.default_rng(2).permutation(px).astype(np.uint8).reshape(1, 128, 256, 3)


HIST_CASES = {
    "odd sizes, a ragged tail, frames off the 16-byte boundary": _rand((3, 13, 37, 3), 3),
    "every bin exactly once": _every_bin_once(),
    "one colour: every add lands on one bin": np.broadcast_to(np.array([200, 17, 93], dtype=np.uint8), (2, 64, 64, 3)).copy(),
    "pixels that differ in the low three bits only": (np.array([96, 160, 8]) + np.random.default_rng(4).integers(0, 8, size=(1, 31, 45, 3))).astype(np.uint8),
    "three workgroups a frame, more bins than private slots": _rand((2, 100, 173, 3), 5),
    "a smooth frame": np.stack([ref.field_frame(48, 80, f) for f in (0, 1)], 0),
}


@pytest.mark.parametrize("per_frame", [True, False], ids=["per frame", "global"])
@pytest.mark.parametrize("name", list(HIST_CASES))
def test_color_hist_equals_bincount(name, per_frame):
    frames = HIST_CASES[name]
    want = ref.color_hist(frames, per_frame)
    got = _hist(frames, per_frame)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got[..., 0].sum() == frames.size // 3
    assert np.array_equal(_hist(frames, per_frame), got)                    # the same bits on a second call


# ---- the map
def _map(frames, palettes, ncolors, stats=True):
    idx, sse, st = ops.palette_map(_dev(frames), _dev(palettes), ncolors, stats=stats)
    return idx.cpu().numpy(), sse.cpu().numpy(), None if st is None else st.cpu().numpy().view(np.uint32).astype(np.int64)


def _check_map(frames, palettes, ncolors):
    want_idx, want_sse, want_stats = ref.palette_map(frames, palettes, ncolors)
    idx, sse, stats = _map(frames, palettes, ncolors)
    assert np.array_equal(idx, want_idx) and np.array_equal(sse, want_sse) and np.array_equal(stats, want_stats)
    idx2, sse2, none = _map(frames, palettes, ncolors, stats=False)          # the launch without the per-entry sums
    assert none is None and np.array_equal(idx2, want_idx) and np.array_equal(sse2, want_sse)
    return idx


@pytest.mark.parametrize("ncolors", [1, 2, 255, 256])
def test_palette_map_equals_the_brute_force_argmin(ncolors):
    frames = _rand((3, 13, 37, 3), 6)
    idx = _check_map(frames, _rand((3, 256, 3), 7 + ncolors), [ncolors] * 3)
    assert idx.max() < ncolors
    _check_map(frames, _rand((3, 256, 3), 8), [ncolors, 1 + ncolors // 2, 256])      # another count per frame


def test_ties_go_to_the_lowest_index():
    pal = np.zeros((1, 256, 3), dtype=np.uint8)
    pal[0, :6] = [[40, 10, 10], [10, 10, 10], [20, 10, 10], [10, 10, 10], [20, 10, 10], [10, 30, 10]]      # 1 == 3, 2 == 4
    px = np.array([[10, 10, 10], [20, 10, 10], [15, 10, 10], [30, 10, 10], [10, 20, 10], [25, 10, 10], [10, 10, 40]], dtype=np.uint8)
    frames = px[np.random.default_rng(9).integers(0, len(px), size=(2, 17, 23))]
    frames.reshape(-1, 3)[:len(px)] = px
    idx = _check_map(frames, pal, [6])
    got = {tuple(p): int(idx.reshape(-1)[i]) for i, p in enumerate(px)}
    # half-way between entries 1 and 2 -> 1; between 2 and 0 -> 0; between 1 and 5 -> 1; the duplicates 3 and 4 are never chosen
    assert got == {(10, 10, 10): 1, (20, 10, 10): 2, (15, 10, 10): 1, (30, 10, 10): 0, (10, 20, 10): 1, (25, 10, 10): 2, (10, 10, 40): 1}
    assert not np.isin(idx, [3, 4]).any()


def test_every_frame_reads_its_own_palette_and_one_palette_serves_all():
    frames = _rand((3, 13, 37, 3), 10)
    base = _rand((256, 3), 11)
    rng = np.random.default_rng(12)
    perms = [rng.permutation(256) for _ in range(3)]
    pals = np.stack([base[p] for p in perms], 0)
    idx = _check_map(frames, pals, [256] * 3)
    one = _check_map(frames, base[None], [256])                             # npal = 1 with n = 3
    for f in range(3):
        assert np.array_equal(pals[f][idx[f]], base[one[f]])                # the same colours whatever the order (no two entries are equal)
    assert len({tuple(c) for c in base}) == 256


def test_entries_beyond_ncolors_are_never_chosen():
    rng = np.random.default_rng(13)
    colours = _rand((150, 3), 14)
    frames = colours[rng.integers(0, 150, size=(3, 13, 37))]
    pals = _rand((3, 256, 3), 15)
    pals[:, 100:250] = colours                                               # every pixel's own colour, behind the last candidate
    idx = _check_map(frames, pals, [100, 7, 1])
    assert idx[0].max() < 100 and idx[1].max() < 7 and idx[2].max() == 0


# ---- Lloyd iterations and the whole of quantize_frames
def _video(n, h, w, sigma, seed):
    rng = np.random.default_rng(seed)
    return np.stack([ref.field_frame(h, w, f, sigma, rng) for f in range(n)], 0)


@pytest.mark.parametrize("palette,colors", [("frame", 256), ("global", 256), ("frame", 64)])
def test_four_lloyd_iterations_equal_the_restatement_and_keep_the_derived_bound(palette, colors):
    frames = _video(2, 48, 80, 6.0, 16)
    want_idx, want_pal, want_n, want_sse, trail = ref.quantize(frames, colors, palette, refine=4)
    runs = [export.quantize_frames(_dev(frames), colors=colors, palette=palette, refine=r) for r in range(5)]
    q = runs[4]
    assert np.array_equal(q.indices, want_idx) and np.array_equal(q.palettes, want_pal) and np.array_equal(q.ncolors, want_n)
    assert np.array_equal(q.frame_sse, want_sse) and q.palette == palette
    for r in range(4):
        assert np.array_equal(runs[r].frame_sse, trail[r])                   # the sum each iteration started from
    pixels = 48 * 80
    for before, after in zip(runs[:-1], runs[1:]):
        print("sse per frame:", before.frame_sse, "->", after.frame_sse, "bound +", 0.75 * pixels)
        if palette == "frame":
            assert (after.frame_sse <= before.frame_sse + 0.75 * pixels).all()
        assert after.frame_sse.sum() <= before.frame_sse.sum() + 0.75 * pixels * 2
    assert np.array_equal(q.frame_psnr, 10 * np.log10(255.0 ** 2 / (q.frame_sse / (pixels * 3.0))))
    assert np.array_equal(q.frames(), np.stack([want_pal[f if palette == "frame" else 0][want_idx[f]] for f in range(2)], 0))


def _decode(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    return im, [np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)]


@pytest.mark.parametrize("palette", ["frame", "global"])
def test_write_gif_end_to_end_from_device_and_host_frames(palette, tmp_path):
    frames = _video(5, 48, 80, 4.0, 17)
    buf = io.BytesIO()
    q = export.write_gif(_dev(frames), buf, duration=0.05, loop=0, palette=palette, refine=1)
    im, decoded = _decode(buf.getvalue())
    assert im.n_frames == 5 and im.size == (80, 48) and im.info["duration"] == 50 and im.info["loop"] == 0
    assert q.palettes.shape == ((5 if palette == "frame" else 1), 256, 3) and q.indices.shape == (5, 48, 80)
    assert np.array_equal(np.stack(decoded, 0), q.frames())
    assert np.array_equal(q.frame_sse, ((q.frames().astype(np.int64) - frames) ** 2).reshape(5, -1).sum(1))
    # host copies of the same frames -- a numpy array, a list of PIL images, floats in [0, 1] -- give the same bytes
    from PIL import Image
    path = tmp_path / "host.gif"
    h = export.write_gif(frames, str(path), duration=0.05, loop=0, palette=palette, refine=1)
    assert path.read_bytes() == buf.getvalue()
    for other in (export.quantize_frames([Image.fromarray(f) for f in frames], palette=palette, refine=1),
                  export.quantize_frames((frames / 255.0).astype(np.float32), palette=palette, refine=1),
                  export.quantize_frames(_dev(frames)[None], palette=palette, refine=1), h):
        assert np.array_equal(other.indices, q.indices) and np.array_equal(other.palettes, q.palettes)
        assert np.array_equal(other.ncolors, q.ncolors) and np.array_equal(other.frame_sse, q.frame_sse)


def test_few_colours_are_reproduced_exactly():
    rng = np.random.default_rng(18)
    bins = rng.choice(ref.BINS, size=40, replace=False)                      # one colour per bin, at most 256 of them: nothing is lost
    colours = (np.stack([((bins >> s) & 31) << 3 for s in (10, 5, 0)], 1) + rng.integers(0, 8, size=(40, 3))).astype(np.uint8)
    frames = colours[rng.integers(0, 40, size=(2, 21, 35))]
    q = export.quantize_frames(_dev(frames))
    assert (q.frame_sse == 0).all() and np.array_equal(q.frames(), frames) and (q.frame_psnr == np.inf).all()
    assert (q.ncolors <= 40).all()


# ---- quality: no lower than Pillow's own median cut of the same frame; no margin
@pytest.mark.parametrize("sigma", [0.0, 6.0, 20.0])
def test_quality_is_no_lower_than_pillows_median_cut(sigma):
    from PIL import Image
    frame = ref.field_frame(256, 384, 2, sigma, np.random.default_rng(0))
    pil = np.asarray(Image.fromarray(frame).quantize(256, Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB"))
    theirs = ref.psnr(pil, frame)
    dev = _dev(frame[None])
    q0, q4 = export.quantize_frames(dev, refine=0), export.quantize_frames(dev, refine=4)
    print(f"sigma {sigma}: Pillow {theirs:.3f} dB, refine=0 {q0.frame_psnr[0]:.3f} dB, refine=4 {q4.frame_psnr[0]:.3f} dB")
    assert q0.frame_psnr[0] == ref.psnr(q0.frames()[0], frame)              # the exact error sum is the decoded frame's
    assert q0.frame_psnr[0] >= theirs
    assert q4.frame_psnr[0] >= q0.frame_psnr[0]

"""CPU: the host half of the GIF export.  tt_palette_median_cut against the numpy restatement (tests/gif_reference.py) entry for entry,
with the partition and colour-range invariants; the files export.write_gif_indexed writes from host indices and palettes, read back
by Pillow (an independent decoder); the refusals of the two device entry points (in a child process that sees no GPU) and of
tt_gif_lzw; and gif_host.cpp under the address and undefined-behaviour sanitizers in a stand-alone program."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gif_reference as ref
from tests import gif_refusals as refusals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _hist(bins, rng, maxcount=50):
    """a histogram with the given occupied bins: 1 .. maxcount pixels each, every pixel's channels inside its bin"""
    bins = np.asarray(bins, dtype=np.int64)
    h = np.zeros((ref.BINS, 4), dtype=np.int64)
    n = rng.integers(1, maxcount + 1, size=bins.size)
    h[bins, 0] = n
    for c, shift in enumerate((10, 5, 0)):
        low = ((bins >> shift) & 31) << 3
        h[bins, 1 + c] = n * low + np.array([rng.integers(0, 8, size=k).sum() for k in n])
    return h


def _cube(side, count):
    """side^3 neighbouring bins of `count` pixels each at their bins' lowest colours: every box count and every extent ties"""
    r, g, b = np.mgrid[4:4 + side, 9:9 + side, 20:20 + side]
    bins = ((r << 10) | (g << 5) | b).reshape(-1)
    h = np.zeros((ref.BINS, 4), dtype=np.int64)
    h[bins, 0] = count
    h[bins, 1], h[bins, 2], h[bins, 3] = count * (r.reshape(-1) << 3), count * (g.reshape(-1) << 3), count * (b.reshape(-1) << 3)
    return h


def _cases():
    rng = np.random.default_rng(5)
    pick = lambda k: rng.choice(ref.BINS, size=k, replace=False)
    return {
        "5000 bins": (_hist(pick(5000), rng), 256),
        "all bins": (_hist(np.arange(ref.BINS), rng, 4), 256),
        "256 bins": (_hist(pick(256), rng), 256),
        "257 bins": (_hist(pick(257), rng), 256),
        "one bin": (_hist(pick(1), rng), 256),
        "2 colors": (_hist(pick(5000), rng), 2),
        "16 colors": (_hist(pick(5000), rng), 16),
        "ties: a cube of equal bins": (_cube(4, 7), 256),
        "ties: a cube of equal bins, 16 colors": (_cube(4, 7), 16),
        "ties: counts of 1": (_hist(pick(3000), rng, 1), 256),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_median_cut_equals_the_numpy_restatement(lib, name):
    from this_and_that_vdm_amd import export
    hist, colors = CASES[name]
    want_pal, want_n, want_boxes = ref.median_cut(hist, colors)
    pal, n, box = export.median_cut(hist.astype(np.uint32), colors, boxes=True)
    occupied = np.nonzero(hist[:, 0])[0]
    assert n == want_n == min(colors, occupied.size)
    assert np.array_equal(pal, want_pal)
    # the boxes partition the occupied bins (and are the restatement's) ...
    assert (box[hist[:, 0] == 0] == -1).all() and (box[occupied] >= 0).all() and (box[occupied] < n).all()
    for k, members in enumerate(want_boxes):
        assert np.array_equal(np.nonzero(box == k)[0], np.sort(members)), k
    # ... and every entry lies inside its box's colour range
    for k in range(n):
        members = np.nonzero(box == k)[0]
        assert members.size
        for c, shift in enumerate((10, 5, 0)):
            coord = (members >> shift) & 31
            assert (coord.min() << 3) <= pal[k, c] <= (coord.max() << 3) + 7, (k, c)
    assert not pal[n:].any()


def test_one_colour_per_bin_is_reproduced_exactly(lib):
    from this_and_that_vdm_amd import export
    rng = np.random.default_rng(6)
    bins = rng.choice(ref.BINS, size=256, replace=False)
    colours = np.stack([((bins >> s) & 31) << 3 for s in (10, 5, 0)], 1) + rng.integers(0, 8, size=(256, 3))
    frame = colours[rng.integers(0, 256, size=(1, 40, 50))].astype(np.uint8)
    frame.reshape(-1, 3)[:256] = colours                                   # every colour at least once
    pal, n = export.median_cut(ref.color_hist(frame)[0].astype(np.uint32), 256)
    assert n == 256
    idx, sse, _ = ref.palette_map(frame, pal[None], [n])
    assert sse[0] == 0 and np.array_equal(pal[idx[0]], frame[0])
    assert export.median_cut(ref.color_hist(frame[:, :1, :1])[0].astype(np.uint32), 256)[1] == 1


# ---- LZW and the container, read back by Pillow
def _read_back(data):
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    frames = [np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)]
    durations = []
    for i in range(im.n_frames):
        im.seek(i)
        durations.append(im.info.get("duration"))
    return im, frames, durations


def _roundtrip(indices, palettes, ncolors, **kw):
    from this_and_that_vdm_amd import export
    buf = io.BytesIO()
    export.write_gif_indexed(indices, palettes, ncolors, buf, **kw)
    data = buf.getvalue()
    im, frames, durations = _read_back(data)
    f, h, w = indices.shape
    assert im.n_frames == f and im.size == (w, h)
    for i in range(f):
        assert np.array_equal(frames[i], palettes[i if palettes.shape[0] == f else 0][indices[i]]), i
    return data, im, durations


def _palettes(rng, n, ncolors):
    pal = np.zeros((n, 256, 3), dtype=np.uint8)
    for i in range(n):
        pal[i, :ncolors] = rng.integers(0, 256, size=(ncolors, 3))
    return pal


def test_random_indices_fill_and_reset_the_table(lib):
    from this_and_that_vdm_amd import export
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 256, size=(2, 96, 96)).astype(np.uint8)
    data, im, durations = _roundtrip(idx, _palettes(rng, 2, 256), [256, 256], duration=0.05, loop=0)
    assert durations == [50, 50] and im.info.get("loop") == 0
    back, clears, widest, used = ref.lzw_decode(export.lzw_frame(idx[0], 8))
    assert np.array_equal(back, idx[0].reshape(-1))
    assert clears >= 3 and widest == 12, (clears, widest)                  # the first clear code and more than one reset; 12-bit codes


def test_a_constant_frame_and_a_single_pixel(lib):
    from this_and_that_vdm_amd import export
    rng = np.random.default_rng(8)
    const = np.full((1, 200, 300), 9, dtype=np.uint8)
    data, _, _ = _roundtrip(const, _palettes(rng, 1, 10), [10])
    assert len(data) < 1200                                                # 60 000 pixels in long runs: ~350 codes
    back, clears, _, _ = ref.lzw_decode(export.lzw_frame(const[0], 4))
    assert np.array_equal(back, const.reshape(-1)) and clears == 1
    _roundtrip(np.zeros((1, 1, 1), dtype=np.uint8), _palettes(rng, 1, 1), [1])
    _roundtrip(np.ones((3, 1, 1), dtype=np.uint8), _palettes(rng, 3, 2), [2, 2, 2])


@pytest.mark.parametrize("ncolors,bits,mcs", [(2, 1, 2), (3, 2, 2), (17, 5, 5), (256, 8, 8)])
def test_table_padding_and_minimum_code_sizes(lib, ncolors, bits, mcs):
    rng = np.random.default_rng(9 + ncolors)
    idx = rng.integers(0, ncolors, size=(2, 13, 37)).astype(np.uint8)
    idx[0, 0, :2] = [0, ncolors - 1]
    data, _, _ = _roundtrip(idx, _palettes(rng, 2, ncolors), [ncolors, ncolors], loop=3, duration=0.1)
    # header 6 + screen 7 + NETSCAPE 19 + control 8 = 40: the first image descriptor, its local table, the min-code-size byte
    assert data[40] == 0x2c and data[49] == 0x80 | (bits - 1) and data[50 + 3 * (1 << bits)] == mcs
    assert not any(data[50 + 3 * ncolors:50 + 3 * (1 << bits)])            # the padding is zeros


def test_a_global_palette_file_loop_none_and_durations(lib):
    rng = np.random.default_rng(10)
    idx = rng.integers(0, 100, size=(3, 20, 31)).astype(np.uint8)
    pal = _palettes(rng, 1, 100)
    data, im, durations = _roundtrip(idx, pal, [100], duration=0.12, loop=None)
    assert data[10] == 0x80 | 0x70 | 6 and data[13:13 + 300] == pal[0, :100].tobytes() and not any(data[313:13 + 3 * 128])
    assert data[13 + 384] == 0x21 and data[14 + 384] == 0xf9               # no NETSCAPE block: the first graphic control follows the table
    assert "loop" not in im.info and durations == [120, 120, 120]
    assert b"NETSCAPE2.0" not in data
    data, im, durations = _roundtrip(idx, pal, [100], duration=0.001, loop=5)
    assert im.info.get("loop") == 5 and durations == [10, 10, 10]          # rounded, and never 0: one centisecond
    with open(os.devnull, "wb") as fh:                                     # a file object and a path are both served
        from this_and_that_vdm_amd import export
        export.write_gif_indexed(idx, pal, [100], fh)


def test_write_gif_indexed_refuses_what_it_cannot_write(lib):
    from this_and_that_vdm_amd import export
    idx = np.zeros((2, 4, 4), dtype=np.uint8)
    pal = np.zeros((2, 256, 3), dtype=np.uint8)
    for bad in (dict(indices=idx[0]), dict(palettes=pal[:, :255]), dict(ncolors=[1]), dict(ncolors=[1, 257]), dict(ncolors=[0, 1]),
                dict(indices=idx + 1), dict(loop=-1), dict(palette="global"), dict(palette="local")):
        kw = dict(dict(indices=idx, palettes=pal, ncolors=[1, 1], path_or_file=io.BytesIO()), **bad)
        with pytest.raises(ValueError, match="write_gif"):
            export.write_gif_indexed(**kw)


# ---- refusals
def test_every_refusal_of_the_device_entry_points_precedes_the_device():
    got = refusals.run_child()
    for family, rows in (("hist", refusals.HIST_ROWS), ("map", refusals.MAP_ROWS)):
        for fault, code, fragment in rows:
            rc, msg = got[refusals.row_id(family, fault)]
            assert rc == code and fragment in msg, (family, fault, rc, msg)
            assert msg.startswith("tt_color_hist:" if family == "hist" else "tt_palette_map:"), msg


def test_lzw_refusals_and_a_buffer_that_is_too_small(lib):
    idx = np.random.default_rng(11).integers(0, 256, size=5000).astype(np.uint8)
    cap = lib.tt_gif_lzw_bound(idx.size)
    out = np.full(cap + 64, 0xAB, dtype=np.uint8)
    n = ctypes.c_int64(-1)
    assert lib.tt_gif_lzw(idx.ctypes.data, idx.size, 8, out.ctypes.data, cap, ctypes.byref(n)) == 0 and 0 < n.value <= cap
    need = n.value
    for small in (0, 1, 2, need // 2, need - 1):
        out[:] = 0xAB
        assert lib.tt_gif_lzw(idx.ctypes.data, idx.size, 8, out.ctypes.data, small, ctypes.byref(n)) == refusals.EINVAL
        assert b"too small" in lib.tt_last_error() and (out[small:] == 0xAB).all()       # an error, not an overrun
    assert lib.tt_gif_lzw(idx.ctypes.data, idx.size, 8, out.ctypes.data, need, ctypes.byref(n)) == 0 and n.value == need
    for args, fragment in (((None, 5, 8, out.ctypes.data, cap), b"null indices"), ((idx.ctypes.data, 5, 8, None, cap), b"null out"),
                           ((idx.ctypes.data, 0, 8, out.ctypes.data, cap), b"npix = 0"),
                           ((idx.ctypes.data, 5, 1, out.ctypes.data, cap), b"min_code_size = 1"),
                           ((idx.ctypes.data, 5, 9, out.ctypes.data, cap), b"min_code_size = 9"),
                           ((idx.ctypes.data, idx.size, 7, out.ctypes.data, cap), b"does not fit min_code_size 7")):
        assert lib.tt_gif_lzw(*args, ctypes.byref(n)) == refusals.EINVAL and fragment in lib.tt_last_error(), fragment
    assert lib.tt_gif_lzw_bound(0) == 0 and lib.tt_gif_lzw_bound(1) >= 6


def test_quantize_frames_refuses_before_it_touches_a_device():
    from this_and_that_vdm_amd import export
    rgb = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    for frames, kw, fragment in ((rgb[..., :1], {}, "3 channels"), (np.zeros((2, 8, 8, 4), dtype=np.uint8), {}, "3 channels"),
                                 (np.zeros((2, 2, 8, 8, 3), dtype=np.uint8), {}, "one video per file"), (rgb, dict(colors=0), "colors"),
                                 (rgb, dict(colors=257), "colors"), (rgb, dict(palette="local"), "palette"), (rgb, dict(refine=-1), "refine"),
                                 (rgb.astype(np.int32), {}, "uint8 or floating-point"), ([], {}, "empty list")):
        with pytest.raises(ValueError, match=fragment):
            export.quantize_frames(frames, **kw)


# ---- the host code under the sanitizers, on its own
def test_gif_host_under_address_and_undefined_sanitizers(tmp_path):
    """gif_host.cpp, lib.cpp (tt_set_error) and tests/gif_host_check.cpp (its own main) built with the host compiler and run as a child
    process: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "gif_host_check")
    # the runtimes are linked INTO the program (clang's default; gcc needs the two flags): it then runs whatever else the environment
    # has the loader bring in first
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "gif_host_check.cpp"), os.path.join(csrc, "gif_host.cpp"),
           os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

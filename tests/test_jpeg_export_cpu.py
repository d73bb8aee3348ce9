"""CPU: the format and the host half of the JPEG export.  The restatement of tests/jpeg_reference.py against Pillow's baseline encoder
(libjpeg-turbo) -- the entropy-coded scan and the DQT payloads byte for byte, 4:4:4 and 4:2:0, grey and RGB --; that the chosen cases
really hold what they are for (a stuffed FF, a ZRL symbol, a block without EOB, an EOB-only block, the DC categories, dummy blocks, the
replicated chroma row); tt_jpeg_quant_tables at every quality, the standard and the optimized Huffman tables of the library; the
refusals of the two device entry points (in a child process that sees no GPU) and of export.encode_jpeg; jpeg_host.cpp under the
address and undefined-behaviour sanitizers in a stand-alone program; and the Motion-JPEG container on the restatement's files.

Everything here is equality: baseline JPEG as libjpeg writes it is integer arithmetic from end to end.  (The kernel divides in the
quantiser and uses no reciprocal, so there is no reciprocal table to check.)"""
import io
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import jpeg_reference as ref
from tests import jpeg_refusals as refusals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (8, 24), (24, 8), (9, 17), (17, 9), (15, 33), (24, 40), (37, 53), (64, 96)]


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _pillow_jpeg():
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("the installed Pillow has no JPEG support")


def _pillow(frame, quality, sub, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, optimize=False, **kw)
    return buf.getvalue()


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def _equal_to_pillow(frame, quality, sub):
    mine, theirs = ref.jpeg_file(frame, quality, sub), _pillow(frame, quality, sub)
    assert ref.segments_of(mine)[1] == ref.segments_of(theirs)[1], "the scans differ"
    assert ref.dqt_payloads(mine) == ref.dqt_payloads(theirs), "the DQT payloads differ"
    return mine, theirs


# ---- the restatement against Pillow
@pytest.mark.parametrize("ch", [3, 1], ids=["rgb", "grey"])
@pytest.mark.parametrize("sub", [ref.S444, ref.S420], ids=["444", "420"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restatements_scan_and_dqt_equal_pillows(size, sub, ch):
    _pillow_jpeg()
    h, w = size
    for quality in (10, 75, 95):
        for frame in (ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 1, ch)):
            mine, theirs = _equal_to_pillow(frame, quality, sub)
            if ch == 3:
                assert mine == theirs                       # with the standard tables the whole file is Pillow's
            else:                                           # (Pillow's SOF0 repeats the subsampling on a grey frame's one component: no effect)
                assert np.array_equal(_decode(mine), _decode(theirs))


EXTREMES = {
    "noise 37x53": lambda ch: ref.noise_frame(37, 53, 2, ch), "checkerboard 24x40": lambda ch: ref.checker_frame(24, 40, ch),
    "flat 0 9x9": lambda ch: ref.flat_frame(9, 9, 0, ch), "flat 255 9x9": lambda ch: ref.flat_frame(9, 9, 255, ch),
    "smooth 64x96": lambda ch: ref.smooth_frame(64, 96, 3, ch),
}


@pytest.mark.parametrize("ch", [3, 1], ids=["rgb", "grey"])
@pytest.mark.parametrize("sub", [ref.S444, ref.S420], ids=["444", "420"])
@pytest.mark.parametrize("name", list(EXTREMES))
def test_the_extreme_qualities_equal_pillows(name, sub, ch):
    _pillow_jpeg()
    for quality in (1, 5, 100):
        _equal_to_pillow(EXTREMES[name](ch), quality, sub)


def test_pillows_plain_save_is_quality_75_in_420():
    _pillow_jpeg()
    from PIL import Image
    frame = ref.smooth_frame(37, 53, 4)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG")
    assert buf.getvalue() == ref.jpeg_file(frame, 75, ref.S420)


def test_the_restatements_tables_are_the_ones_pillow_writes():
    _pillow_jpeg()
    got = ref.dht_tables(_pillow(ref.smooth_frame(16, 16), 75, 0))
    for key, name in ((0x00, "dc_lum"), (0x10, "ac_lum"), (0x01, "dc_chr"), (0x11, "ac_chr")):
        assert got[key] == (ref.STD_BITS[name], ref.STD_VALS[name]), name


# ---- the cases hold what they are for
def _all_symbols(frame, quality, sub):
    coefs, comps, dummy = ref.coefficients(frame, quality, sub)
    return coefs, comps, dummy, ref.symbols(coefs, comps)


def test_the_cases_contain_what_they_are_for():
    # a stuffed FF 00, a block without EOB (its 63rd coefficient is not zero): noise at quality 100
    coefs, comps, _, syms = _all_symbols(ref.noise_frame(37, 53, 2), 100, ref.S444)
    assert b"\xff\x00" in ref.scan_bytes(coefs, comps)
    assert any(int(b[63]) != 0 for b in coefs) and any(blk[-1][:2] != (1, 0) and blk[-1][:2] != (3, 0) for blk in syms)
    # a ZRL symbol (16 zeros): the checkerboard's lone high frequencies at a low quality, or noise at quality 10
    found = False
    for frame, quality in ((ref.checker_frame(24, 40), 75), (ref.noise_frame(37, 53, 2), 10), (ref.noise_frame(64, 96, 1), 10)):
        found = found or any(s == 0xF0 for blk in _all_symbols(frame, quality, ref.S444)[3] for t, s, _, _ in blk if t in (1, 3))
    assert found
    # an EOB-only block and a DC difference of category 0: a flat frame
    coefs, comps, _, syms = _all_symbols(ref.flat_frame(9, 9, 255), 75, ref.S444)
    assert any(len(blk) == 2 and blk[0][1] == 0 and blk[1][1] == 0 for blk in syms)
    # the largest DC category an 8-bit input reaches: 0 next to 255 at quality 100 (Q = 8: DC +-1016 .. 1024, a difference of 11 bits)
    frame = np.concatenate([ref.flat_frame(8, 8, 0), ref.flat_frame(8, 8, 255)], 1)
    coefs, comps, _, syms = _all_symbols(frame, 100, ref.S444)
    assert max(blk[0][1] for blk in syms) == 11
    # dummy Y blocks on the right (8 x 24: two MCUs, the second has one real column) and at the bottom (24 x 8)
    for shape, want in (((8, 24), [False, False, True, True, False, False, False, True, True, True, False, False]),
                        ((24, 8), [False, True, False, True, False, False, False, True, True, True, False, False])):
        coefs, comps, dummy, _ = _all_symbols(ref.noise_frame(*shape, 5), 75, ref.S420)
        assert dummy.tolist() == want
        for i in np.nonzero(dummy)[0]:
            assert coefs[i][0] == coefs[i - 1][0] and not coefs[i][1:].any()
    # a height whose padded chroma rows differ from what repeating the SOURCE rows to the block grid would give.  The two rules differ
    # where the last chroma row is the mean of two DIFFERENT source rows, an even height off the MCU grid (an odd CHROMA height here:
    # 9 rows -> 16, rows 9 .. 15 repeat chroma row 8 = the mean of source rows 16 and 17); with an odd height the last chroma row is
    # the last source row twice and both rules agree, which the sizes 9 x 17, 17 x 9, 15 x 33 and 37 x 53 hold against Pillow above
    frame = ref.noise_frame(18, 16, 6)
    chroma = ref.planes(frame, ref.S420)[1]
    f64 = frame.astype(np.int64)
    cb = (-11059 * f64[..., 0] - 21709 * f64[..., 1] + 32768 * f64[..., 2] + (128 << 16) + 32767) >> 16
    by_source = cb[[17, 17]][:, 0::2] + cb[[17, 17]][:, 1::2]
    by_source = (by_source[0] + by_source[1] + np.where(np.arange(8) % 2 == 0, 1, 2)) >> 2
    assert np.array_equal(chroma[9], chroma[8]) and not np.array_equal(chroma[9], by_source)
    _pillow_jpeg()
    _equal_to_pillow(frame, 75, ref.S420)
    assert ref.planes(ref.noise_frame(9, 17, 6), ref.S420)[1].shape == (8, 16)


# ---- the host routines
def test_quant_tables_of_every_quality_equal_the_restatement(lib):
    from this_and_that_vdm_amd import export
    for quality in range(1, 101):
        got = export.jpeg_quant_tables(quality)
        lum, chrom = ref.quant_tables(quality)
        assert got[0].tolist() == lum and got[1].tolist() == chrom, quality
    assert set(export.jpeg_quant_tables(100).reshape(-1).tolist()) == {1} and int(export.jpeg_quant_tables(1).max()) == 255
    for bad in (0, 101, -5):
        with pytest.raises(RuntimeError, match="quality"):
            export.jpeg_quant_tables(bad)


def _table_properties(table, counts=None):
    codes = ref.codes_of(table.bits, table.huffval)
    assert len(codes) == len(table.huffval) == sum(table.bits)
    assert sum(Fraction(1, 1 << length) for _, length in codes.values()) <= 1                   # Kraft
    for sym, (code, length) in codes.items():
        assert 1 <= length <= 16 and code != (1 << length) - 1, (sym, code, length)            # no all-ones code
        assert int(table.codes[sym]) == (code | length << 16)
    assert all(int(table.codes[s]) == 0 for s in range(256) if s not in codes)
    if counts is not None:
        assert set(codes) == set(np.nonzero(counts)[0].tolist())
        return sum(int(c) * codes[s][1] for s, c in enumerate(counts) if c)


def test_the_standard_tables_are_annex_k(lib):
    from this_and_that_vdm_amd import export
    tables = export.jpeg_standard_tables()
    for table, (bits, vals) in zip(tables, ref.standard_tables()):
        assert table.bits == bits and table.huffval == vals
        _table_properties(table)


COUNT_FRAMES = {"smooth 64x96 q75 420": (lambda: ref.smooth_frame(64, 96, 3), 75, ref.S420), "noise 37x53 q95 444": (lambda: ref.noise_frame(37, 53, 2), 95, ref.S444),
                "noise 37x53 q1": (lambda: ref.noise_frame(37, 53, 2), 1, ref.S420), "flat": (lambda: ref.flat_frame(9, 9, 0), 75, ref.S444),
                "checkerboard q100": (lambda: ref.checker_frame(24, 40), 100, ref.S444)}


@pytest.mark.parametrize("name", list(COUNT_FRAMES))
def test_optimized_tables_are_legal_and_no_worse_than_the_standard_ones(lib, name):
    _pillow_jpeg()
    from this_and_that_vdm_amd import export
    make, quality, sub = COUNT_FRAMES[name]
    frame = make()
    coefs, comps, _ = ref.coefficients(frame, quality, sub)
    counts = ref.symbol_counts(coefs, comps)
    standard = export.jpeg_standard_tables()
    tables = [export.jpeg_optimized_table(counts[k]) for k in range(4)]
    for k in range(4):
        bits = _table_properties(tables[k], counts[k])
        std_codes = ref.codes_of(standard[k].bits, standard[k].huffval)
        assert bits <= sum(int(c) * std_codes[s][1] for s, c in enumerate(counts[k]) if c), k
    mine = ref.jpeg_file(frame, quality, sub, [(t.bits, t.huffval) for t in tables])
    plain = ref.jpeg_file(frame, quality, sub)
    assert len(mine) <= len(plain) and np.array_equal(_decode(mine), _decode(plain))


def test_optimized_table_of_hand_made_counts(lib):
    from this_and_that_vdm_amd import export
    fib = np.zeros(256, dtype=np.int64)
    a, b = 1, 1
    for s in range(40):
        fib[s * 5], a, b = a, b, a + b
    t = export.jpeg_optimized_table(fib)
    _table_properties(t, fib)
    assert max(i + 1 for i, c in enumerate(t.bits) if c) == 15                                   # the limit binds
    one = np.zeros(256, dtype=np.int64)
    one[0x21] = 1                                                                              # ties with the reserved symbol's count
    t = export.jpeg_optimized_table(one)
    assert t.huffval == [0x21] and t.bits[0] == 1 and int(t.codes[0x21]) == (0 | 1 << 16)       # the code 0; the reserved symbol took 1
    assert export.jpeg_optimized_table(np.zeros(256, dtype=np.int64)).huffval == []
    _table_properties(export.jpeg_optimized_table(np.full(256, 3)), np.full(256, 3))
    with pytest.raises(ValueError, match="256 counts"):
        export.jpeg_optimized_table(np.zeros(12))


def test_sizes(lib):
    for (h, w, ch, sub) in [(1, 1, 3, 0), (8, 24, 3, 2), (24, 8, 3, 2), (9, 17, 1, 2), (37, 53, 3, 0), (576, 1024, 3, 2)]:
        blocks = ref.blocks_per_frame(h, w, ch, sub)
        assert lib.tt_jpeg_blocks(h, w, ch, sub) == blocks
        bound = lib.tt_jpeg_scan_bound(h, w, ch, sub)
        assert bound % 16 == 0 and bound >= 2 * (blocks * 64 * 27 // 8) + 2
    assert lib.tt_jpeg_blocks(576, 1024, 3, 0) == 27648
    assert lib.tt_jpeg_blocks(8, 8, 2, 0) == 0 and lib.tt_jpeg_scan_bound(8, 8, 3, 1) == 0 and lib.tt_jpeg_scan_ws_bytes(0, 8, 8, 3, 0) == 0


# ---- refusals
def test_every_refusal_of_the_device_entry_points_precedes_the_device():
    got = refusals.run_child()
    for family, (entry, _, _, rows) in refusals.FAMILIES.items():
        for fault, code, fragment in rows:
            rc, msg = got[refusals.row_id(family, fault)]
            assert rc == code and fragment in msg and msg.startswith(entry + ":"), (family, fault, rc, msg)


def test_encode_jpeg_refuses_before_it_touches_a_device(tmp_path):
    from this_and_that_vdm_amd import export
    rgb = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    for frames, kw, fragment in ((np.zeros((2, 2, 8, 8, 3), dtype=np.uint8), {}, "one video per file"), (rgb, dict(quality=0), "quality"),
                                 (rgb, dict(quality=101), "quality"), (rgb, dict(quality=75.0), "quality"), (rgb, dict(subsampling="4:2:2"), "subsampling"),
                                 (rgb, dict(subsampling=2), "subsampling"), (rgb, dict(huffman="best"), "huffman"),
                                 (rgb.astype(np.int32), {}, "uint8 or floating-point"), ([], {}, "empty list"),
                                 (np.zeros((2, 8, 8, 4), dtype=np.uint8), {}, "JPEG has no alpha"), (np.zeros((2, 8, 8, 2), dtype=np.uint8), {}, "JPEG has no alpha"),
                                 (np.zeros((1, 1, 65536, 1), dtype=np.uint8), {}, "65535 pixels a side")):
        with pytest.raises(ValueError, match=fragment):
            export.encode_jpeg(frames, **kw)
    with pytest.raises(ValueError, match="quality"):
        export.write_jpegs(rgb, str(tmp_path / "never"), quality=200)
    assert not (tmp_path / "never").exists()
    with pytest.raises(ValueError, match="huffman"):
        export.write_mjpeg(rgb, io.BytesIO(), huffman="arithmetic")


# ---- the host code under the sanitizers, on its own
def test_jpeg_host_under_address_and_undefined_sanitizers(tmp_path):
    """jpeg_host.cpp, png_host.cpp (the package-merge), lib.cpp (tt_set_error) and tests/jpeg_host_check.cpp (its own main) built with the
    host compiler and run as a child process: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "jpeg_host_check")
    # the runtimes are linked INTO the program (clang's default; gcc needs the two flags)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "jpeg_host_check.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "png_host.cpp"), os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- the container, on the restatement's files
@pytest.fixture(scope="module")
def clip():
    return [ref.jpeg_file(ref.smooth_frame(24, 40, s), 75, ref.S420) for s in range(3)] + [ref.jpeg_file(ref.noise_frame(24, 40, 9), 75, ref.S420)]


@pytest.mark.parametrize("fps,want", [(4, Fraction(4, 1)), (12.5, Fraction(25, 2)), (Fraction(30000, 1001), Fraction(30000, 1001))], ids=["4", "12.5", "ntsc"])
def test_the_mjpeg_container_round_trips_with_consistent_sizes_and_index(clip, fps, want, tmp_path):
    from this_and_that_vdm_amd import export
    data = export.mjpeg_avi(clip, fps=fps)
    path = str(tmp_path / "clip.avi")
    with open(path, "wb") as fh:
        fh.write(data)
    assert export.read_mjpeg_frames(path) == clip
    info = export.read_mjpeg(data)                                      # the walker checks the RIFF sizes and every idx1 offset and size
    assert info["fps"] == want and info["total_frames"] == info["stream_length"] == 4 and info["streams"] == 1
    assert (info["width"], info["height"]) == (info["strf_width"], info["strf_height"]) == (40, 24)
    assert info["stream_type"] == b"vids" and info["handler"] == b"MJPG" and info["compression"] == b"MJPG" and info["bit_count"] == 24
    assert info["usec_per_frame"] == round(1e6 / float(want))
    assert all(flags == 0x10 for flags, _, _ in info["index"]) and [sz for _, _, sz in info["index"]] == [len(d) for d in clip]
    assert any(len(d) & 1 for d in clip) and len(data) % 2 == 0          # an odd frame is padded: every chunk starts on an even byte
    assert all(off % 2 == 0 for _, off, _ in info["index"])
    assert data[:4] == b"RIFF" and data[8:16] == b"AVI LIST" and data[20:24] == b"hdrl" and data[24:28] == b"avih"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    for d in info["frames"]:
        assert _decode(d).shape == (24, 40, 3)


def test_the_walker_notices_a_broken_container(clip):
    from this_and_that_vdm_amd import export
    data = bytearray(export.mjpeg_avi(clip, fps=4))
    with pytest.raises(ValueError, match="RIFF size"):
        export.read_mjpeg(bytes(data[:-2]))
    at = data.rindex(b"idx1")
    broken = bytearray(data)
    broken[at + 8 + 8:at + 8 + 12] = struct.pack("<I", 6)               # the first entry's offset
    with pytest.raises(ValueError, match="does not point at its chunk"):
        export.read_mjpeg(bytes(broken))
    with pytest.raises(ValueError, match="several sizes"):
        export.mjpeg_avi(clip + [ref.jpeg_file(ref.smooth_frame(8, 8), 75, ref.S420)])
    with pytest.raises(ValueError, match="no frames"):
        export.mjpeg_avi([])

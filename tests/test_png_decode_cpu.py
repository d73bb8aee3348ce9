"""CPU: the PNG import of include/ttvdm.h ("PNG import") before any kernel runs -- the restatement of tests/png_decode_reference.py against
``zlib.decompress`` and Pillow on every stream and file the GPU tests use, its parallel formulations (pointer doubling, the anti-diagonal
wavefront) against its serial ones, tt_png_parse through ``ingest.parse_png`` against the restatement's chunk walk on the files and on
every refusal by name, the device entry points' refusals (they answer before the first HIP call), and the parser under the address and
undefined-behaviour sanitizers in a stand-alone program.  Equality throughout."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_decode_reference as g
from this_and_that_vdm_amd.ingest import decode_png, parse_png, read_apng          # the feature under test: without it nothing here is collected

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_the_restatements_inflate_equals_zlib_and_every_stream_has_the_property_it_is_there_for():
    for name, stream, prop in g.encoder_cases() + g.handbuilt_cases():
        got = g.inflate(stream)
        assert got["status"] == 0 and got["out"] == zlib.decompress(stream), name
        assert prop(got["blocks"]), name + ": the stream no longer has the property the case relies on"
    kinds = [b["kind"] for _, s, _ in g.handbuilt_cases() for b in g.inflate(s)["blocks"]]
    assert {"stored", "fixed", "dynamic"} <= set(kinds)


def test_the_restatement_raises_every_status_bit_on_the_stream_built_for_it():
    seen = 0
    for name, stream, expected, want in g.corrupt_cases():
        got = g.inflate(stream, expected)
        assert got["status"] == want and len(got["out"]) == expected, (name, got["status"])
        seen |= want
        if want & ~(g.SHORT | g.LONG | g.DIST):                      # zlib refuses what the restatement marks as broken data
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
    assert seen == g.BLOCK | g.CODE | g.DIST | g.SHORT | g.LONG | g.ADLER


def test_pillow_refuses_a_flipped_adler_byte_and_loads_a_flipped_idat_crc():
    from PIL import Image
    data = g.pillow_png(g.picture(9, 7, 3, 1))
    hd = g.parse(data)
    stream = bytearray(hd["idat"])
    stream[-1] ^= 1
    with pytest.raises(OSError, match="broken data stream"):
        Image.open(io.BytesIO(g.png_file(7, 9, 2, bytes(stream)))).load()
    at = hd["spans"][0][0] + hd["spans"][0][1]                       # the first IDAT's CRC
    flipped = bytearray(data)
    flipped[at] ^= 0xff
    assert np.array_equal(g.pillow_pixels(bytes(flipped)), g.pillow_pixels(data))


def test_the_restatements_pixels_equal_pillows_on_every_file():
    sizes = []
    for name, data in g.file_cases():
        px, status, rows = g.decode(data)
        assert status == 0 and rows == 0 and np.array_equal(px, g.pillow_pixels(data)), name
        sizes.append(len(g.parse(data)["spans"]))
    files = dict(g.file_cases())
    assert len(g.parse(files["several IDAT chunks"])["spans"]) >= 2, "Pillow no longer cuts IDAT at 65536 bytes"
    assert len(g.inflate(g.parse(files["256 x 384 RGB: several blocks"])["idat"])["blocks"]) >= 2
    assert len(g.parse(files["1-byte IDAT chunks"])["spans"]) > 100
    for name in ("ancillary chunks", "grey with tRNS"):               # Pillow leaves the mode alone for these colour types
        from PIL import Image
        assert Image.open(io.BytesIO(files[name])).mode in ("RGB", "L"), name


def test_pointer_doubling_equals_the_serial_copies_and_a_constant_stream_takes_the_rounds_of_noise():
    for name, stream, _ in g.encoder_cases()[:6] + g.handbuilt_cases():
        got = g.inflate(stream)
        out, _ = g.resolve_by_doubling(g.source_words(got["blocks"]))
        assert out.tobytes() == got["out"], name
    n = 20000
    constant = g.inflate(zlib.compress(bytes(n), 9))
    assert max(g.distances(constant["blocks"])) == 1                  # one chain as long as the stream
    out, rounds = g.resolve_by_doubling(g.source_words(constant["blocks"]))
    assert out.tobytes() == bytes(n)
    assert rounds == g.resolve_by_doubling(g.source_words(g.inflate(zlib.compress(g.noise(n, 1)))["blocks"]))[1] == 15


def test_the_wavefront_equals_the_serial_unfilter():
    rng = np.random.default_rng(0)
    for h, w, ch in ((1, 1, 1), (1, 7, 3), (7, 1, 4), (13, 17, 2), (40, 9, 3)):
        px = g.picture(h, w, ch, h + w, smooth=False)
        kinds = [int(k) for k in rng.integers(0, 5, size=h)]
        stream = g.filter_rows(px, kinds)
        serial, bad = g.unfilter(stream, h, w, ch)
        assert bad == 0 and np.array_equal(serial, px) and np.array_equal(g.unfilter_wavefront(stream, h, w, ch), px), (h, w, ch)
    spoiled = bytearray(g.filter_rows(g.picture(3, 4, 1, 1), [1, 2, 3]))
    spoiled[5] = 9                                                    # row 1's type byte
    serial, bad = g.unfilter(bytes(spoiled), 3, 4, 1)
    assert bad == 1 and np.array_equal(serial, g.unfilter_wavefront(bytes(spoiled), 3, 4, 1))


def apng(frames, default_in=True):
    """a tiny APNG writer: every frame covers the canvas, dispose 0, blend 0"""
    h, w, ch = frames[0].shape
    color = {1: 0, 2: 4, 3: 2, 4: 6}[ch]
    out, seq = [g.SIGNATURE, g.chunk(b"IHDR", g.ihdr(w, h, color=color)), g.chunk(b"acTL", struct.pack(">II", len(frames), 0))], 0
    for i, fr in enumerate(frames):
        stream = zlib.compress(g.filter_rows(fr, [i % 5] * h))
        out.append(g.chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, 1, 20, 0, 0)))
        seq += 1
        if i == 0:
            out.append(g.chunk(b"IDAT", stream))
        else:
            for at in range(0, len(stream), 50):
                out.append(g.chunk(b"fdAT", struct.pack(">I", seq) + stream[at:at + 50]))
                seq += 1
    return b"".join(out + [g.chunk(b"IEND", b"")])


def test_parse_png_reads_what_the_restatement_reads(lib):
    files = g.file_cases() + [("animated", apng([g.picture(6, 5, 3, s) for s in range(3)]))]
    for name, data in files:
        want, hd = g.parse(data), parse_png(data)
        assert (hd.height, hd.width, hd.channels, hd.color_type, hd.bit_depth, hd.interlace) == (want["height"], want["width"], want["channels"], want["color_type"], 8, 0), name
        assert [tuple(s) for s in hd.spans.tolist()] == [s[:2] for s in want["spans"]] and hd.span_frames == [s[2] for s in want["spans"]], name
        assert hd.data[hd.idat[0]:hd.idat[0] + hd.idat[1]].tobytes() == want["idat"], name
        assert (hd.plays, hd.announced, hd.default_is_frame, len(hd.frames)) == (want["plays"], want["announced"], want["default_is_frame"], len(want["frames"])), name
        for got, fr in zip(hd.frames, want["frames"]):
            assert all(got[k] == fr[k] for k in ("sequence", "width", "height", "x", "y", "delay_num", "delay_den", "dispose", "blend")), name
            assert hd.data[got["data_offset"]:got["data_offset"] + got["data_bytes"]].tobytes() == bytes(fr["data"]), name


def test_every_refusal_of_the_parser_names_its_cause_as_the_restatement_does(lib):
    for name, data, fragment in g.refusal_files():
        with pytest.raises(ValueError) as mine:
            g.parse(data)
        assert fragment in str(mine.value), name
        with pytest.raises(ValueError) as e:
            parse_png(data)
        assert fragment in str(e.value) and str(e.value).startswith("tt_png_parse:"), (name, str(e.value))
        with pytest.raises(ValueError) as e:
            decode_png(data, "cuda:0")                                 # refused by the parser: no device is touched
        assert str(e.value).startswith("decode_png: file 0: tt_png_parse:") and fragment in str(e.value), name
    with pytest.raises(ValueError, match="decode_png: decodes on the HIP device, got cpu"):
        decode_png(g.file_cases()[0][1], "cpu")
    a, b = g.pillow_png(g.picture(4, 5, 3, 1)), g.pillow_png(g.picture(4, 5, 4, 1))
    with pytest.raises(ValueError, match="file 1 is 4 x 5 x 4, file 0 is 4 x 5 x 3"):
        decode_png([a, b], "cuda:0")
    with pytest.raises(ValueError, match="not an animated PNG"):
        read_apng(a, "cuda:0")
    region = apng([g.picture(6, 5, 3, s) for s in range(2)])
    at = region.rindex(b"fcTL") + 4                                   # the second fcTL: width 4 at x = 1
    region = region[:at + 4] + struct.pack(">I", 4) + region[at + 8:at + 12] + struct.pack(">I", 1) + region[at + 16:]
    with pytest.raises(ValueError, match=r"frame 1's fcTL names the region 4 x 6 at \(1, 0\)"):
        read_apng(region, "cuda:0")
    blend = apng([g.picture(6, 5, 3, s) for s in range(2)])
    at = blend.rindex(b"fcTL") + 4 + 25
    with pytest.raises(ValueError, match="frame 1's fcTL names dispose 0 / blend 1"):
        read_apng(blend[:at] + b"\1" + blend[at + 1:], "cuda:0")


def test_the_device_entry_points_refuse_before_the_first_hip_call(lib):
    from this_and_that_vdm_amd import _lib
    buf = np.zeros(4096, dtype=np.uint8)
    at = buf.ctypes.data
    at += -at % 16
    good = dict(data=at, data_bytes=100, offsets=at, lengths=at, expected=at, out_offsets=at, n=2, max_out=50, out=at, out_bytes=128, status=at, ws=at, ws_bytes=1 << 20, stream=None)
    order = list(good)

    def inflate(**kw):
        rc = lib.tt_png_inflate(*[{**good, **kw}[k] for k in order])
        return rc, lib.tt_last_error().decode()

    rows = [(dict(data=None), -1, "null data"), (dict(ws=None), -1, "null ws"), (dict(n=0), -1, "empty problem"), (dict(max_out=0), -1, "empty problem"),
            (dict(max_out=129), -1, "max_out = 129 above out_bytes"), (dict(offsets=at + 4), -1, "offsets is not 8-byte aligned"),
            (dict(expected=at + 2), -1, "expected is not 4-byte aligned"), (dict(ws=at + 8), -1, "ws is not 16-byte aligned"),
            (dict(ws_bytes=100), -1, "ws too small"), (dict(n=65536), -2, "65536 streams"), (dict(data_bytes=1 << 29), -2, "32-bit bit offsets"),
            (dict(out_bytes=1 << 31), -2, "fewer than 2^31")]
    einval, eunsupported = inflate(data=None)[0], inflate(n=65536)[0]
    assert einval != 0 and eunsupported not in (0, einval)
    for change, kind, fragment in rows:
        rc, msg = inflate(**change)
        assert rc == (einval if kind == -1 else eunsupported) and fragment in msg and msg.startswith("tt_png_inflate:"), (change, rc, msg)
    # the workspace is the derived bound: n records of 32 bytes, a word per byte of out, a pair per chunk; 0 for what is refused
    assert lib.tt_png_decode_ws_bytes(3, 10000, 5000) == 96 + 40000 + 16 * (3 * 2 * 8 // 16)
    assert [lib.tt_png_decode_ws_bytes(*a) for a in ((0, 10, 10), (65536, 10, 10), (1, 0, 1), (1, 1 << 31, 1), (1, 10, 11), (1, 10, 0))] == [0] * 6
    for change, fragment in ((dict(filtered=None), "null filtered"), (dict(ch=5), "ch = 5"), (dict(h=0), "h = 0"), (dict(filtered=at + 8), "filtered is not 16-byte aligned"),
                             (dict(n=65536), "65536 frames")):
        args = {**dict(filtered=at, n=1, h=4, w=5, ch=3, out=at, status=at, stream=None), **change}
        assert lib.tt_png_unfilter(*args.values()) != 0 and fragment in lib.tt_last_error().decode(), change


def test_png_host_under_address_and_undefined_sanitizers(tmp_path):
    """png_host.cpp, lib.cpp and tests/png_decode_host_check.cpp (its own main) built with the host compiler and run as a child process:
    nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "png_decode_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "png_decode_host_check.cpp"), os.path.join(csrc, "png_host.cpp"),
           os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])

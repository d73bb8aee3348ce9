"""CPU: the format and the host half of the JPEG import.  The restatement of tests/jpeg_decode_reference.py against Pillow's decoder
(libjpeg-turbo), pixel for pixel -- RGB 4:4:4 and 4:2:0 and grey, standard and optimized tables, odd sizes, the qualities 1 to 100,
smooth, noise, checkerboard and flat frames, the 640 x 480 fixture --; its decoded coefficients against the export's restatement; the
emulation of the parallel entropy decoder (rule 4's lanes and passes) against the plain sequential decoder; tt_jpeg_parse through
ctypes: a good file field by field, every refusal by its text on a file with one field edited, truncated files; tt_jpeg_decode_table
for the standard and an optimized table; and both host routines under the address and undefined-behaviour sanitizers in a stand-alone
program.

Everything here is equality: a baseline JPEG decodes in integers from end to end."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_reference as dec
from tests import jpeg_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "bridge_task1_im_0.jpg")
SIZES = [(1, 1), (8, 8), (8, 24), (24, 8), (8, 9), (9, 17), (17, 9), (18, 33), (40, 41), (50, 34), (37, 53), (64, 96)]
NARROW = [(9, 3), (9, 1), (5, 4), (12, 2), (7, 5)]          # chroma planes of one and two columns: libjpeg repeats the samples there


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _pillow(frame, quality, sub, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, **kw)
    return buf.getvalue()


def _pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def _frames(h, w, ch):
    return {"smooth": ref.smooth_frame(h, w, 1, ch), "noise": ref.noise_frame(h, w, 2, ch), "checker": ref.checker_frame(h, w, ch),
            "flat 0": ref.flat_frame(h, w, 0, ch), "flat 255": ref.flat_frame(h, w, 255, ch)}


# ---- the restatement against Pillow
@pytest.mark.parametrize("kind", ["4:4:4", "4:2:0", "grey"])
@pytest.mark.parametrize("size", SIZES + NARROW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restatement_decodes_pillows_files_to_pillows_pixels(size, kind):
    h, w = size
    ch, sub = (1, 0) if kind == "grey" else (3, ref.SUBSAMPLING[kind])
    for name, frame in _frames(h, w, ch).items():
        for quality in (1, 10, 75, 95, 100):
            for optimize in (False, True):
                data = _pillow(frame, quality, sub, optimize=optimize)
                got, status = dec.decode(data)
                want = _pillow_pixels(data)
                assert status == 0 and np.array_equal(got, want), (name, quality, optimize, np.argwhere(got != want)[:5])


def test_the_restatement_decodes_the_fixture_to_pillows_pixels():
    with open(FIXTURE, "rb") as fh:
        data = fh.read()
    assert len(data) == 104362
    got, status = dec.decode(data)
    assert status == 0 and got.shape == (480, 640, 3) and np.array_equal(got, _pillow_pixels(data))


def test_the_edge_rule_is_visible_at_the_odd_sizes():
    """clamping the upsampler's neighbours at the padded plane instead of the real ceil(h / 2) x ceil(w / 2) samples changes pixels"""
    for h, w in ((8, 9), (40, 41), (50, 34)):
        hd = dec.parse(_pillow(ref.noise_frame(h, w, 2), 95, 2))
        coeffs, _ = dec.entropy_sequential(hd["scan"], dec.decode_set(hd), hd["dc"], hd["ac"], h, w, 3, ref.S420)
        plane = dec._plane(dec.block_samples(coeffs.reshape(-1, 6, 64)[:, 4], hd["quant"][1]), -(-h // 16), -(-w // 16))
        real, padded = dec.upsample_h2v2(plane, -(-h // 2), -(-w // 2)), dec.upsample_h2v2(plane, *plane.shape)
        assert not np.array_equal(real[:h, :w], padded[:h, :w]), (h, w)


# ---- coefficients, and the parallel scheme
CASES = [((37, 53), ref.S420, 75, 3), ((37, 53), ref.S444, 100, 3), ((8, 24), ref.S420, 10, 3), ((24, 8), ref.S420, 95, 3), ((9, 17), ref.S444, 75, 1), ((64, 96), ref.S444, 95, 3)]


@pytest.mark.parametrize("size,sub,quality,ch", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_decoded_coefficients_equal_the_exports_and_the_lanes_equal_the_sequential_decoder(size, sub, quality, ch):
    h, w = size
    for frame in (ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch)):
        for optimize in (False, True):
            hd = dec.parse(_pillow(frame, quality, sub, optimize=optimize))
            args = (hd["scan"], dec.decode_set(hd), hd["dc"], hd["ac"], h, w, ch, sub)
            coeffs, status = dec.entropy_sequential(*args)
            assert status == 0 and np.array_equal(coeffs, ref.coefficients(frame, quality, sub)[0])
            for S in (128, 1024):
                for lanes in (4, 256):
                    got, st, passes = dec.entropy_lanes(*args, S, lanes)
                    assert st == 0 and np.array_equal(got, coeffs), (S, lanes)
                    assert len(passes) == -(-8 * len(dec.unstuff(hd["scan"])[0]) // (S * lanes)) and max(passes) <= lanes


def test_the_lanes_agree_with_the_sequential_decoder_on_broken_streams():
    """a scan cut short, a scan with flipped bits, a scan with bytes appended: the same coefficients and the same status, never a hang"""
    frame = ref.noise_frame(37, 53, 5)
    hd = dec.parse(_pillow(frame, 90, 2))
    rest = (dec.decode_set(hd), hd["dc"], hd["ac"], 37, 53, 3, ref.S420)
    scan = hd["scan"]
    rng = np.random.default_rng(7)
    broken = [scan[:len(scan) // 2], scan[:len(scan) - 3], scan + b"\x12\x34\x56", scan[:1], b""]
    for _ in range(6):
        b = bytearray(scan)
        for at in rng.integers(0, len(b), size=3):
            b[at] ^= 1 << int(rng.integers(0, 8))
        broken.append(bytes(b))
    for i, s in enumerate(broken):
        c0, s0 = dec.entropy_sequential(s, *rest)
        for S, lanes in ((128, 16), (1024, 256), (64, 4)):
            c1, s1, _ = dec.entropy_lanes(s, *rest, S, lanes)
            assert s1 == s0 and np.array_equal(c1, c0), (i, S, lanes)
        if i < 5:
            assert s0 != 0, i


# ---- tt_jpeg_parse
def _parse(lib, data):
    import ctypes as C
    from this_and_that_vdm_amd import _lib
    hd = _lib.TtJpegHeader()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = lib.tt_jpeg_parse(buf.ctypes.data if buf.size else None, buf.size, C.byref(hd))
    return rc, lib.tt_last_error().decode(), hd


@pytest.mark.parametrize("kind", ["4:4:4", "4:2:0", "grey"])
def test_parse_reads_what_the_restatement_reads(lib, kind):
    ch, sub = (1, 2) if kind == "grey" else (3, ref.SUBSAMPLING[kind])
    for optimize in (False, True):
        data = _pillow(ref.noise_frame(37, 53, 2, ch), 90, sub, optimize=optimize, comment=b"skipped")
        rc, msg, hd = _parse(lib, data)
        want = dec.parse(data)
        assert rc == 0, msg
        assert (hd.h, hd.w, hd.ch, hd.subsampling) == (37, 53, ch, want["sub"])
        assert data[hd.scan_offset:hd.scan_offset + hd.scan_bytes] == want["scan"] and data[hd.scan_offset + hd.scan_bytes:] == b"\xff\xd9"
        assert list(hd.dc_table)[:ch] == want["dc"] and list(hd.ac_table)[:ch] == want["ac"]
        assert [list(q) for q in hd.quant][:ch] == want["quant"]
        for slot, key in enumerate((0x00, 0x10, 0x01, 0x11)):
            bits, vals = want["tables"].get(key, ([0] * 16, []))
            assert list(hd.bits[slot]) == bits and list(hd.huffval[slot])[:len(vals)] == vals, slot


def _find(data, marker):
    at = 2
    while data[at + 1] != marker:
        at += 2 + struct.unpack(">H", data[at + 2:at + 4])[0]
    return at


def _edit(data, marker, offset, value):
    """the file with the byte at ``offset`` of the first ``marker`` segment's payload replaced"""
    out = bytearray(data)
    out[_find(data, marker) + 4 + offset] = value
    return bytes(out)


def _insert(data, before_marker, segment):
    at = _find(data, before_marker)
    return data[:at] + segment + data[at:]


def test_parse_refuses_by_name(lib):
    good = _pillow(ref.smooth_frame(16, 16, 1), 75, 2)
    grey = _pillow(ref.smooth_frame(16, 16, 1, 1), 75, 0)                       # a grey file defines the tables 0 only
    assert _parse(lib, good)[0] == 0 and _parse(lib, grey)[0] == 0
    sof = _find(good, 0xc0)
    retag = lambda m: good[:sof + 1] + bytes([m]) + good[sof + 2:]
    sos_len = struct.unpack(">H", good[_find(good, 0xda) + 2:_find(good, 0xda) + 4])[0]
    scan_at = _find(good, 0xda) + 2 + sos_len
    dqt16 = bytearray(_edit(good, 0xdb, 0, 0x10))
    rows = [
        (retag(0xc1), -2, "extended sequential"), (retag(0xc2), -2, "progressive"), (retag(0xc9), -2, "arithmetic"),
        (_pillow(ref.smooth_frame(16, 16, 1), 75, 2, progressive=True), -2, "progressive"),
        (_edit(good, 0xc0, 0, 12), -2, "12-bit"),
        (_insert(good, 0xda, b"\xff\xdd\x00\x04\x00\x08"), -2, "restart"),
        (good[:scan_at + 20] + b"\xff\xd0" + good[scan_at + 20:], -2, "restart marker"),
        (good[:-2] + good[_find(good, 0xda):], -2, "several scans"),
        (_edit(good, 0xda, 0, 1)[:_find(good, 0xda) + 2] + b"\x00\x08\x01\x01\x00\x00\x3f\x00" + good[scan_at:], -2, "several scans"),
        (_edit(good, 0xc0, 7, 0x21), -2, "sampling 2x1"), (_edit(good, 0xc0, 10, 0x22), -2, "sampling"),
        (_pillow(ref.smooth_frame(16, 16, 1), 75, 1), -2, "4:2:2"),
        (bytes(dqt16), -2, "16-bit DQT"),
        (_edit(good, 0xc0, 5, 4), -2, "four components"),
        (_insert(good, 0xdb, b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"), -2, "Adobe APP14"),
        (_edit(good, 0xc0, 8, 3), -2, "missing quantiser table 3"),
        (_edit(good, 0xc4, 0, 0x01), -2, "missing DC Huffman table 0"),
        (_edit(grey, 0xda, 2, 0x01), -2, "missing AC Huffman table 1"),
        (_edit(good, 0xda, 2, 0x20), -2, "Huffman table index 2"),
        (_edit(good, 0xda, 8, 5), -2, "progressive"),
        (good[:-2], -1, "ends before EOI"), (good[:scan_at + 10], -1, "ends before EOI"), (good[:scan_at], -1, "ends before EOI"),
        (good[:sof + 6], -1, "ends before"), (good[:3], -1, "ends before"), (b"\x89PNG" + good[4:], -1, "no SOI"),
        (good[:2] + b"\xff\xd9", -1, "ends before its scan"),
    ]
    for i, (data, code, fragment) in enumerate(rows):
        rc, msg, _ = _parse(lib, data)
        assert rc == code and fragment in msg and msg.startswith("tt_jpeg_parse:"), (i, fragment, rc, msg)
    assert _parse(lib, b"")[0] == -1
    # what is skipped: APPn and COM segments, fill bytes before a marker
    rc, msg, hd = _parse(lib, _insert(_insert(good, 0xdb, b"\xff\xe1\x00\x08Exif\x00\x00"), 0xc0, b"\xff\xff\xff\xfe\x00\x05abc"))
    assert rc == 0 and (hd.h, hd.w) == (16, 16), msg


def test_ingest_refuses_before_it_touches_a_device(lib):
    from this_and_that_vdm_amd import ingest
    with pytest.raises(ValueError, match="progressive"):
        ingest.parse_jpeg(_pillow(ref.smooth_frame(16, 16, 1), 75, 2, progressive=True))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ingest.decode_jpeg([_pillow(ref.smooth_frame(16, 16, 1), 75, 2)], "cpu")
    with pytest.raises(ValueError, match="no files"):
        ingest.decode_jpeg([], "cuda")
    with pytest.raises(ValueError, match="file 1: tt_jpeg_parse: .*4:2:2"):
        ingest.decode_jpeg([_pillow(ref.smooth_frame(16, 16, 1), 75, 2), _pillow(ref.smooth_frame(16, 16, 1), 75, 1)], "cuda")
    with pytest.raises(ValueError, match="one geometry and subsampling per call"):
        ingest.decode_jpeg([_pillow(ref.smooth_frame(16, 16, 1), 75, 2), _pillow(ref.smooth_frame(16, 16, 1), 75, 0)], "cuda")
    with pytest.raises(ValueError, match="does not exist"):
        ingest.read_jpegs(os.path.join(REPO, "tests", "golden", "no such clip"))


# ---- tt_jpeg_decode_table
def _lookup(table, code, length):
    """(length, symbol) the kernel's two steps find for ``code`` of ``length`` bits followed by zeros, or None"""
    v16 = code << (16 - length)
    idx = v16 >> 8
    e = (int(table[idx >> 1]) >> (16 * (idx & 1))) & 0xffff
    if e >> 8:
        return e >> 8, e & 255
    for l in range(9, 17):
        c = v16 >> (16 - l)
        if c <= int(table[128 + l:129 + l].view(np.int32)[0]):
            at = (c + int(table[145 + l])) & 255
            return l, (int(table[192 + (at >> 2)]) >> (8 * (at & 3))) & 255
    return None


def test_decode_tables_of_the_standard_and_an_optimized_table(lib):
    from this_and_that_vdm_amd import export, ingest
    coefs, comps, _ = ref.coefficients(ref.noise_frame(37, 53, 2), 95, ref.S444)
    counts = ref.symbol_counts(coefs, comps)
    for t in export.jpeg_standard_tables() + [export.jpeg_optimized_table(counts[1]), export.jpeg_optimized_table(counts[2])]:
        table = ingest.jpeg_decode_table(t.bits, t.huffval)
        assert table.shape == (256,) and table.dtype == np.uint32
        codes = ref.codes_of(t.bits, t.huffval)
        for sym, (code, length) in codes.items():
            assert _lookup(table, code, length) == (length, sym), (sym, code, length)
        longest = max(length for _, length in codes.values())
        assert _lookup(table, (1 << 16) - 1, 16) is None and longest <= 16            # the all-ones pattern is no code
    s = ingest.jpeg_decode_set(export.jpeg_standard_tables())
    assert s.shape == (1028,) and int(s[1024]) == 0b111100 and not s[1025:].any()
    with pytest.raises(RuntimeError, match="oversubscribes"):
        ingest.jpeg_decode_table([3] + [0] * 15, [1, 2, 3])
    with pytest.raises(ValueError, match="16 BITS"):
        ingest.jpeg_decode_table([1] * 15, [1])


# ---- the host code under the sanitizers, on its own
def test_jpeg_decode_host_under_address_and_undefined_sanitizers(tmp_path):
    """jpeg_host.cpp, png_host.cpp, lib.cpp and tests/jpeg_decode_host_check.cpp (its own main) built with the host compiler and run as a
    child process: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "jpeg_decode_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "jpeg_decode_host_check.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "png_host.cpp"), os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
